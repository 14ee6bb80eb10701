"""Case tables of tests/test_nhwc_support_gpu.py: one row per dispatch branch and loop trip of the fp32 NHWC kernels behind the
classification models and the HRNet-OCR head (csrc/hrnet_ops.hip, bn_nhwc.hip with bn_nhwc_core.h and bn_select.h, dense_ops.hip), the seeded
inputs of each row, its float64 reference written out in plain numpy, and a per-element absolute bound for every output.

A row holds `op`, `id`, `kernel` (the name the launcher must note, None where the entry point makes no choice), the
shape, `views` (operand -> (float offset, ld) inside a wider buffer), flags, and `plan`: the trip counts it claims, which
tests/test_nhwc_support_host.py holds to the launch plans restated below.  Nothing here touches the device or the library.

Bounds.  Every bound is a sum of named terms:
  * gamma(L + k) * sum |terms| for an fp32 chain of L additions (L from the plan) and k operand roundings; fp64 stages add nothing;
  * u * |stored statistic| * sensitivity where the kernel re-reads a statistic that was rounded to fp32 (backward rows are handed
    the reference's own forward outputs rounded to fp32);
  * E * u * (1 + |argument|) * |value| for every expf / logf, E = 4: a stated budget, not a measurement.
An output a kernel only moves or selects (a maximum, an identity source, a quarter of a gradient) has bound 0: bit for bit.

Near zero.  The backward rows get the reference's y rounded to fp32, whose sign is the float64 pre-activation's, so no ReLU-mask
element has to be left out (sign_agrees() says so for every row; the host test asserts it).  Bilinear coordinates are fp32 in
the kernel and exact here: every sampled element carries |largest neighbour difference| * 4u * (I - 1) per axis in its bound,
whichever side of an integer the fp32 coordinate falls on, so none is left out either.
"""
import numpy as np

from _plumbing_cases import OFFSET, U, gamma, ids, offc, rng_of  # noqa: F401  (ids: re-exported for the tests)
from _plumbing_cases import q as _q

E = 4.0                 # expf / logf budget, in units of u * (1 + |argument|) * |value|
BN_EPS = float(np.float32(1e-5))        # the entry points take eps and momentum as fp32
BN_MOM = float(np.float32(0.1))
LEFT_OUT_CAP = 1e-3     # at most 0.1 % of any output may be left out of a comparison (nothing is: see above)


def q(a):
    return _q(a, "f32").astype(np.float64)


CASES = []


def case(op, cid, kernel, **kw):
    c = dict(op=op, id=f"{op}:{cid}", kernel=kernel, **kw)
    c.setdefault("views", {})
    c.setdefault("flags", {})
    c.setdefault("plan", {})
    CASES.append(c)
    return c


def cases_of(*ops):
    return [c for c in CASES if c["op"] in ops]


# ================================================================================================== launch plans, restated
OCR_TILE, OCR_MAX_K, OCR_LDS_LIMIT = 64, 32, 64 * 1024
ROWS, TPB, FL = 128, 256, 16


def ocr_chunks(HW):
    """hrnet_ops.hip ocr_chunks: `pc = ceil(HW / OCR_TILE)`, `if (pc > 32) pc = 32`,
    `per = ceil(ceil(HW / pc) / OCR_TILE) * OCR_TILE`, `count = ceil(HW / per)` -> (per, count)."""
    pc = min((HW + OCR_TILE - 1) // OCR_TILE, 32)
    per = ((HW + pc - 1) // pc + OCR_TILE - 1) // OCR_TILE * OCR_TILE
    return per, (HW + per - 1) // per


def ocr_pixels_per_block(HW):
    """hrnet_ops.hip ocr_pixels_per_block: `per = (HW + 127) / 128; per = (per + 7) / 8 * 8`."""
    return ((HW + 127) // 128 + 7) // 8 * 8


def grid_for(total):
    """bn_select.h bn_grid: `b = ceil(total / BN_TPB)`, `b < 1 ? 1 : (b > BN_CAP ? BN_CAP : b)`, BN_CAP = 8192."""
    return min(max((total + TPB - 1) // TPB, 1), 8192)


def nrb(M):
    """bn_select.h bn_row_blocks: `(M + BN_ROWS - 1) / BN_ROWS`."""
    return (M + ROWS - 1) // ROWS


def vec4_ok(C, views):
    """bn_select.h with es = 4: `C % (16 / es)` refuses (bn_channels_ok), then every non-null view whose `ld * es % 16` or whose base
    is not 16-byte aligned does (bn_view_ok).
    views: (float offset inside an allocation that is itself 16-byte aligned, ld) or None."""
    return C % 4 == 0 and all(v is None or (v[1] % 4 == 0 and v[0] % 4 == 0) for v in views)


def pad4(n):
    return (n + 3) // 4 * 4


def ocr_gather_workspace(N, HW, K, C):
    """kd_ocr_gather_workspace: `(pad4(N * count * K * 2) + N * count * K * C) * sizeof(float)`."""
    cnt = ocr_chunks(HW)[1]
    return (pad4(N * cnt * K * 2) + N * cnt * K * C) * 4


def ocr_attend_workspace(N, HW, K, Ck):
    """kd_ocr_attend_workspace: `(2 * pad4(N * HW * K) + 2 * N * count * K * Ck) * sizeof(float)`."""
    cnt = ocr_chunks(HW)[1]
    return (2 * pad4(N * HW * K) + 2 * N * cnt * K * Ck) * 4


def bn_workspace(M, C):
    """bn_select.h bn_workspace: `(nrb * 3 * C + 2 * C) * sizeof(float)`."""
    return (nrb(M) * 3 * C + 2 * C) * 4


def gather_bwd_lds_ok(K, C):
    """kd_ocr_gather_bwd: `K * C * sizeof(float) <= OCR_LDS_LIMIT`."""
    return K * C * 4 <= OCR_LDS_LIMIT


def attend_lds_ok(K, Ck):
    """attend_check: `2 * K * Ck * sizeof(float) <= OCR_LDS_LIMIT`."""
    return 2 * K * Ck * 4 <= OCR_LDS_LIMIT


def ocr_plan(HW):
    """Trip counts of the OCR kernels at HW pixels.
    stats_trips: `for (p = p0 + threadIdx.x; p < p1; p += 256)` of ocr_stats_kernel in a full chunk;
    tiles: `for (t0 = p0; t0 < p1; t0 += OCR_TILE)` of ocr_contract_kernel in a full chunk; last: pixels of the last chunk;
    ppb / blocks / last_block: the per-pixel kernels' blocks; bwd_trips: `for (pa = p0 + wave * 2; pa < p1; pa += 8)` of
    ocr_gather_bwd_kernel; attend_trips: `for (p = p0 + wave; p < p1; p += 4)` of ocr_attend_kernel."""
    per, cnt = ocr_chunks(HW)
    ppb = ocr_pixels_per_block(HW)
    blocks = (HW + ppb - 1) // ppb
    full = min(per, HW)
    return dict(per=per, chunks=cnt, last=HW - (cnt - 1) * per, stats_trips=(full + 255) // 256, tiles=(full + OCR_TILE - 1) // OCR_TILE,
                ppb=ppb, blocks=blocks, last_block=HW - (blocks - 1) * ppb, bwd_trips=(min(ppb, HW) + 7) // 8,
                attend_trips=(min(ppb, HW) + 3) // 4)


def bn_plan(M, C, V):
    """nrb; finish_trips: `for (rb = ty; rb < g.nrb; rb += FL)` of bn_nhwc_stats_finish_kernel (chain 0); bwd_chain / bwd_empty:
    longest `rb += 4` chain of bn_nhwc_grad_finish_kernel and how many of its 4 chains are empty; grid / trips: the
    grid-stride loop `i += gridDim.x * TPB` of the elementwise kernels over M * C / V items."""
    n = nrb(M)
    total = M * (C // V)
    g = grid_for(total)
    return dict(nrb=n, finish_trips=(n + FL - 1) // FL, bwd_chain=(n + 3) // 4, bwd_empty=max(4 - n, 0), grid=g,
                trips=(total + g * TPB - 1) // (g * TPB))


def pool_plan(items, C, V):
    total = items * (C // V)
    g = grid_for(total)
    return dict(grid=g, trips=(total + g * TPB - 1) // (g * TPB))


# ====================================================================================================================== OCR
def _og(cid, shape, plan=None, **kw):
    for op in ("ocr_gather", "ocr_gather_bwd"):
        if op == "ocr_gather_bwd" and not gather_bwd_lds_ok(shape[2], shape[3]):
            continue
        case(op, cid, None, shape=shape, plan=plan or {}, **kw)


_og("min-1px-1class", (1, 1, 1, 4), dict(chunks=1, blocks=1, last=1))
_og("one-chunk-one-tile", (2, 64, 19, 40), dict(chunks=1, per=64, tiles=1))
_og("two-chunks-second-1px", (2, 65, 19, 40), dict(chunks=2, per=64, last=1))
_og("K32", (2, 77, 32, 40), dict(chunks=2))
_og("K32-C512-lds-64KiB", (1, 77, 32, 512), dict(chunks=2))
_og("hw1024-ppb8", (2, 1024, 19, 8), dict(ppb=8, bwd_trips=1))
_og("hw1025-ppb16", (2, 1025, 19, 8), dict(ppb=16, bwd_trips=2, blocks=65, last_block=1))
_og("hw2048-32-chunks", (2, 2048, 5, 8), dict(chunks=32, per=64, tiles=1))
_og("hw2113-two-tiles", (2, 2113, 5, 8), dict(chunks=17, per=128, tiles=2, last=65))
_og("hw8192-one-stats-trip", (1, 8192, 3, 4), dict(per=256, chunks=32, stats_trips=1))
_og("hw8257-two-stats-trips", (1, 8257, 3, 4), dict(per=320, chunks=26, stats_trips=2, last=257))
_og("views", (2, 77, 19, 40), views=dict(logits=(0, 32), feats=(8, 64)))
_og("hw2113-spread30", (2, 2113, 5, 8), dict(chunks=17, tiles=2), flags=dict(spread=30.0))


def _oa(cid, shape, plan=None, **kw):
    for op in ("ocr_attend", "ocr_attend_bwd"):
        case(op, cid, None, shape=shape, plan=plan or {}, **kw)


_oa("min", (1, 1, 1, 4), dict(blocks=1))
_oa("K2", (2, 77, 2, 8))
_oa("K32-Ck256-lds-64KiB", (2, 77, 32, 256))
_oa("K19-Ck428-largest", (2, 77, 19, 428))
_oa("hw1025-four-trips", (2, 1025, 19, 32), dict(ppb=16, attend_trips=4, last_block=1))
_oa("hw2113-two-tiles", (1, 2113, 5, 8), dict(tiles=2, chunks=17))
_oa("views", (2, 77, 19, 32), views=dict(query=(8, 48), g=(4, 40)))
_oa("scale0.37", (2, 77, 5, 8), flags=dict(scale=0.37))
_oa("spread30", (2, 77, 19, 32), flags=dict(spread=30.0))

# refused shapes: (op, shape); the forward gather accepts the first
REFUSALS = [("ocr_gather_bwd", (1, 77, 32, 516)), ("ocr_attend", (1, 77, 32, 260)), ("ocr_attend", (1, 77, 19, 432))]


def _softmax_hw(lg):
    mx = lg.max(1)
    s = np.exp(lg - mx[:, None]).sum(1)
    lse = mx + np.log(s)
    a = lg - lse[:, None]
    return mx, s, lse, a, np.exp(a)


def build_ocr_gather(c):
    r = rng_of(dict(id=c["id"].split(":", 1)[1]))         # forward and backward rows of one id share their data
    N, HW, K, C = c["shape"]
    sp = c["flags"].get("spread")
    lg = r.uniform(-sp, sp, (N, HW, K)) if sp else r.standard_normal((N, HW, K))
    per, cnt = ocr_chunks(HW)
    top = np.abs(lg).max() + 3.0
    lg[:, HW - 1, 0] = top                                # class 0's maximum sits at the last pixel
    if cnt > 1 and K > 1:
        lg[:, per, 1] = top                               # class 1's at the first pixel of the second chunk
    lg, f = q(lg), q(r.standard_normal((N, HW, C)))
    mx, s, lse, a, p = _softmax_hw(lg)
    ref = dict(mx=mx, lse=lse, ctx=np.einsum("npk,npc->nkc", p, f), s=s, a=a, p=p)
    inp = dict(logits=lg, feats=f)
    if c["op"] == "ocr_gather_bwd":
        g = q(r.standard_normal((N, K, C)))
        inp.update(gctx=g, ctx=q(ref["ctx"]), lse=q(lse))
        dk = (g * ref["ctx"]).sum(2)
        dot = np.einsum("npc,nkc->npk", f, g)
        ref.update(d_feats=np.einsum("npk,nkc->npc", p, g), d_logits=p * (dot - dk[:, None]), dot=dot, dk=dk)
    return inp, ref


def _contract_chain(HW):
    """ocr_contract_kernel + ocr_contract_finish_kernel: a wave adds every 4th pixel of its chunk (`j += 4` in each of per / 64
    tiles: per / 4 fmas), three adds join the waves (`f4_add(f4_add(f4_add(...`), the finish adds `chunks` partials to 0."""
    per, cnt = ocr_chunks(HW)
    return per // 4 + 3 + cnt


def _dot_chain(C):
    """`for (c = lane * 4; c < C; c += 256) s += f4_dot(...)`: ceil(C / 256) trips of 4 terms, then wave_sum's 6 levels."""
    return 4 * ((C + 255) // 256) + 6


def bounds_ocr_gather(c, inp, ref):
    N, HW, K, C = c["shape"]
    pl = ocr_plan(HW)
    lg, f, p, a = inp["logits"], inp["feats"], ref["p"], ref["a"]
    # (max, sum) pairs: a value passes at most Lm lse_merge calls (stats_trips in its thread, 6 shuffles, 3 waves, chunks - 1 in
    # ocr_stats_finish_kernel); each is two products and an add (3u) and rescales by one expf whose arguments add up to
    # l - max along the way: E u (Lm + |l - max|) for the value, weighted by its share p of the sum
    Lm = pl["stats_trips"] + 6 + 3 + (pl["chunks"] - 1)
    rel_s = Lm * (3 + E) * U + E * U * (p * np.abs(lg - ref["mx"][:, None])).sum(1)
    # lse = max + logf(sum): the sum's relative error, logf's budget, the add
    b_lse = rel_s + E * U * (1 + ref["s"]) * np.abs(np.log(ref["s"])) + U * np.abs(ref["lse"])
    out = dict(mx=np.zeros_like(ref["mx"]), lse=b_lse)
    # p = expf(l - lse): the subtraction (u |a| in the argument), expf's budget, the kernel's own lse
    rel_p = U * np.abs(a) + E * U * (1 + np.abs(a))
    if c["op"] == "ocr_gather":
        S = np.einsum("npk,npc->nkc", p, np.abs(f))
        out["ctx"] = gamma(_contract_chain(HW) + 1) * S + np.einsum("npk,npc->nkc", p * rel_p, np.abs(f)) + b_lse[..., None] * S
        return out
    # backward: lse is the stored fp32 one (u |lse| in the argument of every expf)
    g = inp["gctx"]
    rel_p = rel_p + U * np.abs(ref["lse"])[:, None]
    # d_feats = sum_k p_k gctx_k: K fmas (`da = f4_fma(pka[k], g, da)`)
    b_df = np.einsum("npk,nkc->npc", p * (gamma(K) + rel_p), np.abs(g))
    # d_logits = p (<gctx_k, f> - dk_k): both dots by _dot_chain (ocr_rowdot_kernel, `dpa[k] += f4_dot(fa, g)`), ctx stored in
    # fp32 (u sum |gctx ctx|), the subtraction, p's error and the product
    Ld = _dot_chain(C)
    absdk = np.abs(g * ref["ctx"]).sum(2)[:, None]
    b_dl = p * (gamma(Ld + 1) * (np.einsum("npc,nkc->npk", np.abs(f), np.abs(g)) + absdk) + U * absdk + U * np.abs(ref["dot"] - ref["dk"][:, None])) \
        + np.abs(ref["d_logits"]) * (rel_p + 2 * U)
    return dict(d_feats=b_df, d_logits=b_dl)


def _scale_of(c):
    return float(np.float32(c["flags"].get("scale", float(c["shape"][3]) ** -0.5)))


def build_ocr_attend(c):
    r = rng_of(dict(id=c["id"].split(":", 1)[1]))
    N, HW, K, Ck = c["shape"]
    sc = _scale_of(c)
    qy, key, val = q(r.standard_normal((N, HW, Ck))), r.standard_normal((N, K, Ck)), q(r.standard_normal((N, K, Ck)))
    if c["flags"].get("spread"):
        key = key * (c["flags"]["spread"] / np.abs(sc * np.einsum("npc,nkc->npk", qy, key)).max())
    key = q(key)
    s = sc * np.einsum("npc,nkc->npk", qy, key)
    e = np.exp(s - s.max(2, keepdims=True))
    p = e / e.sum(2, keepdims=True)
    inp = dict(query=qy, key=key, value=val, scale=sc)
    ref = dict(ctx=np.einsum("npk,nkc->npc", p, val), s=s, p=p)
    if c["op"] == "ocr_attend_bwd":
        g = q(r.standard_normal((N, HW, Ck)))
        dpv = np.einsum("npc,nkc->npk", g, val)
        pd = (p * dpv).sum(2, keepdims=True)
        ds = sc * p * (dpv - pd)
        inp["g"] = g
        ref.update(d_query=np.einsum("npk,nkc->npc", ds, key), d_key=np.einsum("npk,npc->nkc", ds, qy), d_value=np.einsum("npk,npc->nkc", p, g),
                   dpv=dpv, pd=pd, ds=ds)
    return inp, ref


def bounds_ocr_attend(c, inp, ref):
    N, HW, K, Ck = c["shape"]
    sc, qy, key, val, s, p = abs(inp["scale"]), inp["query"], inp["key"], inp["value"], ref["s"], ref["p"]
    Ld = _dot_chain(Ck)
    # score: the dot (`s[k] += f4_dot(qv, key)`, wave_sum) and the product with scale
    es = gamma(Ld + 1) * sc * np.einsum("npc,nkc->npk", np.abs(qy), np.abs(key))
    # softmax over K (first order in the score errors): dp_k = p_k (ds_k - sum_j p_j ds_j); expf(s - m): the subtraction and the
    # budget; the sum of K terms; the reciprocal and the product
    d = np.abs(s - s.max(2, keepdims=True))
    rel_e = U * d + E * U * (1 + d)
    dp = p * (es + (p * es).sum(2, keepdims=True) + rel_e + (p * rel_e).sum(2, keepdims=True) + gamma(K) + 2 * U)
    if c["op"] == "ocr_attend":
        # ctx = sum_k p_k value_k: K fmas
        return dict(ctx=np.einsum("npk,nkc->npc", dp, np.abs(val)) + gamma(K) * np.einsum("npk,nkc->npc", p, np.abs(val)))
    g, dpv, pd, ds = inp["g"], ref["dpv"], ref["pd"], ref["ds"]
    e_dpv = gamma(Ld) * np.einsum("npc,nkc->npk", np.abs(g), np.abs(val))                     # `dp[k] += f4_dot(gv, value)`
    e_pd = (dp * np.abs(dpv) + p * e_dpv).sum(2, keepdims=True) + gamma(K) * (p * np.abs(dpv)).sum(2, keepdims=True)   # `pd += s[k] * dp[k]`
    # ds = scale * p * (dp - pd): the subtraction, two products
    e_ds = sc * (dp * np.abs(dpv - pd) + p * (e_dpv + e_pd + U * np.abs(dpv - pd))) + 3 * U * np.abs(ds)
    Lc = _contract_chain(HW)
    return dict(d_query=np.einsum("npk,nkc->npc", e_ds, np.abs(key)) + gamma(K) * np.einsum("npk,nkc->npc", np.abs(ds), np.abs(key)),
                d_key=np.einsum("npk,npc->nkc", e_ds, np.abs(qy)) + gamma(Lc + 1) * np.einsum("npk,npc->nkc", np.abs(ds), np.abs(qy)),
                d_value=np.einsum("npk,npc->nkc", dp, np.abs(g)) + gamma(Lc + 1) * np.einsum("npk,npc->nkc", p, np.abs(g)))


# ================================================================================================================= HRNet fuse
# out: (Ho, Wo); srcs: [(H, W)]; size: pass size= (no identity source); need: the backward's mask
HR_GEOM = [("share-H", (9, 13), [(9, 13), (9, 5)], {}),
           ("share-W", (9, 13), [(9, 13), (4, 13)], {}),
           ("one-row", (1, 9), [(1, 9), (1, 4)], {}),
           ("ratio-third", (10, 10), [(10, 10), (4, 4)], {}),        # 3 / 9 rounds in fp32: coordinates fall beside the integers
           ("ratio-32", (33, 65), [(33, 65), (2, 3)], {}),
           ("size-no-identity", (9, 13), [(5, 7), (3, 4)], dict(size=True)),
           ("four-need-last", (9, 13), [(9, 13), (5, 7), (3, 4), (1, 1)], dict(need=(False, False, False, True))),
           ("slices", (9, 13), [(9, 13), (5, 7), (3, 4)], dict(sliced=True)),
           ("N1", (9, 13), [(9, 13), (5, 7)], dict(N=1))]
for _cid, _out, _srcs, _fl in HR_GEOM:
    for _C in (4, 48):
        for _op in ("hr_fuse", "hr_fuse_bwd"):
            case(_op, f"{_cid}-C{_C}", None, shape=(_fl.get("N", 2),) + _out + (_C,), srcs=_srcs, flags=_fl,
                 views=dict(all=(8, _C + 16)) if _fl.get("sliced") else {})


def axis_weights(O, I):
    """(O, I) float64 matrix of align_corners=True bilinear weights with hr_src's clamping, and the exact source coordinates."""
    Wm = np.zeros((O, I))
    x = np.arange(O) * ((I - 1) / (O - 1)) if O > 1 else np.zeros(O)
    i0 = np.minimum(np.floor(x).astype(int), I - 1)
    i1 = np.minimum(i0 + 1, I - 1)
    fr = x - i0
    np.add.at(Wm, (np.arange(O), i0), 1 - fr)
    np.add.at(Wm, (np.arange(O), i1), fr)
    return Wm, x


def coord_slack(I):
    """fp32 coordinate `o * sc` with `sc = (float)(I - 1) / (float)(O - 1)`: two roundings of a value below I - 1; 4u (I - 1)."""
    return 4 * U * (I - 1)


def build_hr_fuse(c):
    r = rng_of(dict(id=c["id"].split(":", 1)[1]))
    N, Ho, Wo, C = c["shape"]
    srcs = [q(r.standard_normal((N, h, w, C))) for h, w in c["srcs"]]
    pre = np.zeros((N, Ho, Wo, C))
    mag = np.zeros((N, Ho, Wo, C))
    coord = np.zeros((N, 1, 1, C))
    for s in srcs:
        H, W = s.shape[1:3]
        if (H, W) == (Ho, Wo):
            pre += s
            mag += np.abs(s)
            continue
        Wh, Ww = axis_weights(Ho, H)[0], axis_weights(Wo, W)[0]
        pre += np.einsum("oh,pw,nhwc->nopc", Wh, Ww, s)
        mag += np.einsum("oh,pw,nhwc->nopc", Wh, Ww, np.abs(s))
        dh = np.abs(np.diff(s, axis=1)).max((1, 2), keepdims=True) if H > 1 else 0.0
        dw = np.abs(np.diff(s, axis=2)).max((1, 2), keepdims=True) if W > 1 else 0.0
        coord = coord + coord_slack(H) * dh + coord_slack(W) * dw
    y = np.maximum(pre, 0)
    inp = dict(srcs=srcs)
    ref = dict(y=y, pre=pre, mag=mag, coord=coord)
    if c["op"] == "hr_fuse_bwd":
        gy = q(r.standard_normal((N, Ho, Wo, C)))
        y32 = q(y)
        gm = gy * (y32 > 0)
        inp.update(gy=gy, y=y32)
        need = c["flags"].get("need", (True,) * len(srcs))
        ref["gsrc"], ref["b_gsrc"] = [], []
        for (H, W), nd in zip(c["srcs"], need):
            if not nd:
                ref["gsrc"].append(None)
                ref["b_gsrc"].append(None)
            elif (H, W) == (Ho, Wo):
                ref["gsrc"].append(gm)                               # `acc = hr_masked(...)`: a move
                ref["b_gsrc"].append(np.zeros_like(gm))
            else:
                (Wh, xh), (Ww, xw) = axis_weights(Ho, H), axis_weights(Wo, W)
                # outputs whose fp32 coordinate may put a corner on source index i: |x - i| < 1 + slack
                Ih = (np.abs(xh[:, None] - np.arange(H)) < 1 + coord_slack(H)).astype(np.float64)
                Iw = (np.abs(xw[:, None] - np.arange(W)) < 1 + coord_slack(W)).astype(np.float64)
                # `acc = f4_fma(wh * ww, g, acc)` over at most L candidates; the weight: 1 - f, the two `+=`, the product
                L = int(Ih.sum(0).max() * Iw.sum(0).max())
                ag = np.abs(gm)
                ref["gsrc"].append(np.einsum("oh,pw,nopc->nhwc", Wh, Ww, gm))
                ref["b_gsrc"].append(gamma(L + 4) * np.einsum("oh,pw,nopc->nhwc", Wh, Ww, ag)
                                     + coord_slack(H) * np.einsum("oh,pw,nopc->nhwc", Ih, Ww, ag)
                                     + coord_slack(W) * np.einsum("oh,pw,nopc->nhwc", Wh, Iw, ag))
    return inp, ref


def bounds_hr_fuse(c, inp, ref):
    if c["op"] == "hr_fuse_bwd":
        return dict(gsrc=ref["b_gsrc"])
    # f4_lerp twice per source (1 - f, two products, an add: 3 roundings each), `acc = f4_add(acc, v)` per further source; the
    # fp32 coordinate; ReLU is 1-Lipschitz
    return dict(y=gamma(6 + len(c["srcs"])) * ref["mag"] + ref["coord"] + np.zeros_like(ref["y"]))


# ======================================================================================================================== BN
BN_SHAPES = [  # (M, C, train, relu): every C on both sides of train / eval and of relu, every M at least once
    (1, 1, True, True), (127, 1, False, False), (128, 3, True, False), (129, 3, False, True), (384, 4, True, True), (513, 4, False, False),
    (2048, 6, True, False), (2049, 6, False, True), (1, 17, False, True), (2049, 17, True, False), (129, 65, True, True),
    (2048, 65, False, False), (127, 68, True, False), (513, 68, False, True)]


def _v(C, views=()):
    return 4 if vec4_ok(C, list(views)) else 1


def _bn(op, cid, M, C, train, relu, views=None, plan=None, **flags):
    views = views or {}
    if op in ("bn_fwd", "bn_apply"):
        vs = [views.get("x"), views.get("y")]
        kern = f"bn_nhwc_apply_kernel<{_v(C, vs)}>"
    elif op == "bn_bwd":
        names = ["gy", "x"] + (["y"] if relu else []) + (["res"] if flags.get("res") else []) + ["dx"]
        kern = f"bn_nhwc_dx_kernel<{_v(C, [views.get(n) for n in names])}>" if flags.get("need_dx", True) else "bn_nhwc_grad_finish_kernel"
    else:
        kern = None
    return case(op, cid, kern, M=M, C=C, train=train, relu=relu, views=views, flags=flags, plan=plan or {})


for _M, _C, _t, _r in BN_SHAPES:
    _tag = f"M{_M}-C{_C}-{'train' if _t else 'eval'}-relu{int(_r)}"
    _pl = {2048: dict(nrb=16, finish_trips=1), 2049: dict(nrb=17, finish_trips=2), 384: dict(nrb=3, bwd_empty=1), 1: dict(nrb=1, bwd_empty=3)}.get(_M, {})
    _bn("bn_fwd", _tag, _M, _C, _t, _r, plan=_pl, run="both")
    _bn("bn_bwd", _tag, _M, _C, _t, _r, plan=_pl, res=_M % 2 == 1)
for _M in (1, 127, 128, 129, 384, 513, 2048, 2049):
    _bn("bn_stats", f"M{_M}-C17", _M, 17, True, False, plan=dict(nrb=nrb(_M)))
_bn("bn_stats", "M513-C8-slice", 513, 8, True, False, views=dict(x=(2, 12)))
# running statistics: none, mean only, variance only, both
for _run in ("none", "mean", "var", "both"):
    _bn("bn_fwd", f"run-{_run}", 384, 4, True, True, run=_run)
    _bn("bn_apply", f"run-{_run}", 129, 4, True, False, run=_run)
_bn("bn_apply", "C6", 129, 6, True, True, run="both")
# the three ways out of vec4_ok, each alone: C = 6 (above); C = 8 in ld 10; C = 8 at float offset 2 of ld 12.  An aligned slice stays <4>
for _name, _view in (("ld10", (0, 10)), ("off2", (2, 12))):
    for _who in ("x", "y"):
        _bn("bn_apply", f"{_name}-on-{_who}", 129, 8, True, True, views={_who: _view}, run="none")
    for _who in ("gy", "x", "y", "res", "dx"):
        _bn("bn_bwd", f"{_name}-on-{_who}", 129, 8, True, True, views={_who: _view}, res=True)
    # y is not read without relu: its view must not keep the call from the float4 kernel
    _bn("bn_bwd", f"{_name}-on-unread-y", 129, 8, True, False, views=dict(y=_view), res=True)
_bn("bn_apply", "aligned-slices", 129, 8, True, True, views=dict(x=(4, 16), y=(8, 24)), run="none")
_bn("bn_bwd", "aligned-slices", 129, 8, True, True, views=dict(gy=(4, 16), x=(8, 24), y=(4, 12), res=(8, 16), dx=(4, 20)), res=True)
_bn("bn_bwd", "C6-res", 129, 6, True, True, res=True)
# flags
_bn("bn_bwd", "eval-dx-only-no-workspace", 129, 8, False, True, res=True, want=())
_bn("bn_bwd", "eval-dx-only-scalar", 129, 6, False, False, want=())
_bn("bn_bwd", "no-dx-dgamma-only", 513, 8, True, True, need_dx=False, want=("dgamma",))
_bn("bn_bwd", "accumulate", 513, 8, True, True, accumulate=True)
_bn("bn_bwd", "accumulate-scalar", 129, 3, True, False, accumulate=True, res=True)
_bn("bn_bwd", "res-aliased-by-out", 129, 8, True, True, res=True, alias=True)
_bn("bn_bwd", "res-aliased-by-out-scalar", 129, 6, True, True, res=True, alias=True)
# the grid-stride second trip: more than 8192 * 256 items
for _C, _V in ((512, 4), (129, 1)):
    _bn("bn_apply", f"big-C{_C}", 16400, _C, True, True, plan=dict(grid=8192, trips=2), run="none", big=True)
    _bn("bn_bwd", f"big-C{_C}", 16400, _C, True, True, plan=dict(grid=8192, trips=2), res=True, big=True)


def _bn_data(c, r):
    M, C = c["M"], c["C"]
    x = r.standard_normal((M, C))
    x[:, offc(C)] += OFFSET
    g, b = q(r.standard_normal(C) * 0.3 + 1), q(r.standard_normal(C) * 0.3)
    rm = r.standard_normal(C) * 0.1
    rm[offc(C)] += OFFSET
    return q(x), g, b, q(rm), q(np.abs(r.standard_normal(C)) + 0.5)


def bn_batch_stats(x):
    """Batch statistics in float64 and the error budget of the two-stage reduction (bn_nhwc_stats_partial_kernel: a thread adds
    ROWS / 4 = 32 values of x - k and of (x - k)^2 around the block's first pixel k, `(a + b) + (c + d)` joins the four lanes: a
    chain of 34; x - k rounds once (s1: +1, s2: +2).  bn_nhwc_stats_finish_kernel is fp64: with s1, s2 per block off by e1, e2 the
    mean moves by sum e1 / M and M2 = sum (s2 - s1^2 / nb) + sum nb (mean_b - mean)^2 by sum (e2 + 2 |k - mean| e1 + e1^2 / nb)."""
    M, C = x.shape
    mean = x.mean(0)
    M2 = ((x - mean) ** 2).sum(0)
    e_mean, e_M2 = np.zeros(C), np.zeros(C)
    for r0 in range(0, M, ROWS):
        blk = x[r0:r0 + ROWS]
        k = blk[0]
        v = blk - k
        e1, e2 = gamma(35) * np.abs(v).sum(0), gamma(36) * (v * v).sum(0)
        e_mean += e1
        e_M2 += e2 + 2 * np.abs(k - mean) * e1 + e1 * e1 / len(blk)
    var = M2 / M
    invstd = 1 / np.sqrt(var + BN_EPS)
    vu = M2 / (M - 1) if M > 1 else var
    return dict(mean=mean, invstd=invstd, var_unb=vu,
                b_mean=e_mean / M + (U * np.abs(mean) if M > 1 else 0.0),     # ... and the fp32 store (M = 1: the mean is k itself)
                b_invstd=0.5 * invstd ** 3 * e_M2 / M + U * invstd,
                b_var_unb=e_M2 / max(M - 1, 1) + U * vu)


def _running(old, new, b_new):
    """bn_running_update: `(1.f - momentum) * running + momentum * v`: 1 - momentum, two products, an add."""
    val = (1 - BN_MOM) * old + BN_MOM * new
    return val, BN_MOM * b_new + gamma(4) * (np.abs((1 - BN_MOM) * old) + np.abs(BN_MOM * new))


def _apply_bound(x, g, b, mean, invstd, d_mean, d_invstd, y_pre):
    """bn_nhwc_apply_kernel: `fmaf(v - mean, gamma * invstd, beta)`: the subtraction, the product gamma * invstd, the fma; mean and
    invstd off by d_mean, d_invstd.  ReLU is 1-Lipschitz."""
    xm = np.abs(x - mean)
    gi = np.abs(g * invstd)
    return gi * (d_mean + U * xm) + xm * np.abs(g) * d_invstd + U * xm * gi + U * np.abs(y_pre)


def build_bn(c):
    r = rng_of(c)
    M, C, op = c["M"], c["C"], c["op"]
    x, g, b, rm, rv = _bn_data(c, r)
    inp = dict(x=x, gamma=g, beta=b, run_mean=rm, run_var=rv)
    st = bn_batch_stats(x) if c["train"] else None
    if op == "bn_stats":
        return inp, dict(st, bounds={k: st["b_" + k] for k in ("mean", "invstd", "var_unb")})
    if c["train"]:
        mean, invstd = st["mean"], st["invstd"]
    else:
        mean, invstd = rm, 1 / np.sqrt(rv + BN_EPS)
    pre = (x - mean) * (g * invstd) + b
    y = np.maximum(pre, 0) if c["relu"] else pre
    ref = dict(y=y, mean=mean, invstd=invstd)
    bd = {}
    if op == "bn_fwd":
        if c["train"]:
            d_mean, d_is = st["b_mean"], st["b_invstd"]
            ref["run_mean"], bd["run_mean"] = _running(rm, mean, d_mean)
            ref["run_var"], bd["run_var"] = _running(rv, st["var_unb"], st["b_var_unb"])
        else:      # bn_nhwc_eval_stats_kernel: the mean is moved, invstd = (float)(1 / sqrt((double)var + eps))
            d_mean, d_is = np.zeros(C), U * invstd
        bd.update(mean=d_mean, invstd=d_is, y=_apply_bound(x, g, b, mean, invstd, d_mean, d_is, pre))
    elif op == "bn_apply":
        # the statistics are handed over, rounded to fp32: u |mean|, u invstd
        inp.update(mean=q(mean), invstd=q(invstd), var_unb=q(st["var_unb"]))
        ref["run_mean"], bd["run_mean"] = _running(rm, mean, U * np.abs(mean))
        ref["run_var"], bd["run_var"] = _running(rv, st["var_unb"], U * st["var_unb"])
        bd["y"] = _apply_bound(x, g, b, mean, invstd, U * np.abs(mean), U * invstd, pre)
    else:
        fl = c["flags"]
        gy = q(r.standard_normal((M, C)))
        y32 = q(y)
        gm = gy * (y32 > 0) if c["relu"] else gy
        xhat = (x - mean) * invstd
        s1, s2 = gm.sum(0), (gm * xhat).sum(0)
        a1, a2 = np.abs(gm).sum(0), np.abs(gm * xhat).sum(0)
        # bn_nhwc_grad_partial_kernel: 32 adds per thread and `(a + b) + (c + d)`: 34; bn_nhwc_grad_finish_kernel is fp64 and stores
        # once.  s2's terms: x - mean, * invstd, the fma; the saved mean and invstd are fp32
        e1 = gamma(35) * a1
        e2 = gamma(38) * a2 + U * np.abs(mean) * invstd * a1 + U * a2
        inp.update(gy=gy, y=y32, mean=q(mean), invstd=q(invstd))
        res = q(r.standard_normal((M, C))) if fl.get("res") else None
        if res is not None:
            inp["res"] = res
        gi = g * invstd
        if c["train"]:
            t = gm - s1 / M - xhat * (s2 / M)
            # `t - sums[c] * inv_m - xhat * (sums[C + c] * inv_m)`: inv_m = (float)(1 / M) and each product round; xhat as above
            e_xhat = invstd * (U * np.abs(mean) + U * np.abs(x - mean)) + 2 * U * np.abs(xhat)
            e_t = (e1 + 2 * U * np.abs(s1)) / M + np.abs(xhat) * (e2 + 2 * U * np.abs(s2)) / M + e_xhat * np.abs(s2) / M \
                + U * np.abs(xhat * s2 / M) + 2 * U * (np.abs(gm) + np.abs(s1 / M) + np.abs(xhat * s2 / M))
        else:
            t, e_t = gm, 0.0
        dx = gi * t
        b_dx = np.abs(gi) * e_t + 3 * U * np.abs(dx)            # `gamma[c] * is * t`: invstd stored in fp32, two products
        if res is not None:
            dx = dx + res
            b_dx = b_dx + U * np.abs(dx)                        # `o[j] += rv[j]`
        dg, db = s2, s1
        if fl.get("accumulate"):
            inp["dgamma0"], inp["dbeta0"] = q(r.standard_normal(C) * 5), q(r.standard_normal(C) * 5)
            dg, db = dg + inp["dgamma0"], db + inp["dbeta0"]
            e2, e1 = e2 + U * np.abs(dg), e1 + U * np.abs(db)   # `dbeta[c] + s1`
        ref = dict(dx=dx, dgamma=dg, dbeta=db, pre=pre, y=y)
        bd = dict(dx=b_dx, dgamma=e2, dbeta=e1)
    ref["bounds"] = bd
    return inp, ref


# ====================================================================================================================== pool
def _pool(op, cid, shape, views=None, plan=None, **flags):
    C = shape[3]
    names = ("x", "y") if op == "avgpool" else ("gy", "gx")
    views = views or {}
    kern = ("avgpool2x2_kernel<%d>" if op == "avgpool" else "avgpool2x2_bwd_kernel<%d>") % _v(C, [views.get(n) for n in names])
    return case(op, cid, kern, shape=shape, views=views, plan=plan or {}, flags=flags)


for _op, _a, _b in (("avgpool", "x", "y"), ("avgpool_bwd", "gy", "gx")):
    _pool(_op, "1x2x2x4", (1, 2, 2, 4))
    _pool(_op, "1x3x2x5", (1, 3, 2, 5))                     # a dropped last row, scalar
    _pool(_op, "2x5x4x6-ld9", (2, 5, 4, 6), views={_a: (0, 9), _b: (0, 9)})
    _pool(_op, "2x5x7x8", (2, 5, 7, 8))                     # a dropped row and column on the float4 kernel
    _pool(_op, "aligned-slices", (2, 5, 4, 8), views={_a: (4, 16), _b: (8, 24)})
    for _name, _view in (("ld10", (0, 10)), ("off2", (2, 12))):
        for _who in (_a, _b):
            _pool(_op, f"{_name}-on-{_who}", (2, 5, 4, 8), views={_who: _view})
# more than 8192 * 256 work items per kernel and per V
_pool("avgpool", "big-v4", (2, 200, 164, 512), plan=dict(grid=8192, trips=2), big=True)
_pool("avgpool", "big-v1", (2, 200, 164, 129), plan=dict(grid=8192, trips=2), big=True)
_pool("avgpool_bwd", "big-v4", (2, 100, 82, 512), plan=dict(grid=8192, trips=2), big=True)
_pool("avgpool_bwd", "big-v1", (2, 101, 83, 129), plan=dict(grid=8192, trips=2), big=True)


def build_pool(c):
    r = rng_of(c)
    N, H, W, C = c["shape"]
    Ho, Wo = H // 2, W // 2
    if c["op"] == "avgpool":
        x = r.standard_normal((N, H, W, C), dtype=np.float32)
        a, b, cc, d = (x[:, i:2 * Ho:2, j:2 * Wo:2].astype(np.float64) for i in (0, 1) for j in (0, 1))
        # `((a + b) + (c + d)) * 0.25f`: two roundings on the way of every term, the quarter is exact
        return dict(x=x), dict(y=(a + b + cc + d) / 4, bounds=dict(y=gamma(2) * (np.abs(a) + np.abs(b) + np.abs(cc) + np.abs(d)) / 4))
    gy = r.standard_normal((N, Ho, Wo, C), dtype=np.float32)
    gx = np.zeros((N, H, W, C))
    gx[:, :2 * Ho, :2 * Wo] = np.repeat(np.repeat(gy.astype(np.float64) / 4, 2, axis=1), 2, axis=2)
    return dict(gy=gy), dict(gx=gx, bounds=dict(gx=np.zeros_like(gx)))        # `v[j] * 0.25f`: exact


# =================================================================================================================== dispatch
def build(c):
    """-> (inputs, reference): float64 numpy arrays holding fp32-representable inputs; reference["bounds"] = {output: bound}."""
    op = c["op"]
    if op.startswith("ocr_gather"):
        inp, ref = build_ocr_gather(c)
        ref["bounds"] = bounds_ocr_gather(c, inp, ref)
    elif op.startswith("ocr_attend"):
        inp, ref = build_ocr_attend(c)
        ref["bounds"] = bounds_ocr_attend(c, inp, ref)
    elif op.startswith("hr_fuse"):
        inp, ref = build_hr_fuse(c)
        ref["bounds"] = bounds_hr_fuse(c, inp, ref)
    elif op.startswith("bn_"):
        inp, ref = build_bn(c)
    else:
        inp, ref = build_pool(c)
    return inp, ref


def bounds(c, ref):
    return ref["bounds"]


OUTPUTS = {"ocr_gather": ("ctx", "mx", "lse"), "ocr_gather_bwd": ("d_feats", "d_logits"), "ocr_attend": ("ctx",),
           "ocr_attend_bwd": ("d_query", "d_key", "d_value"), "hr_fuse": ("y",), "hr_fuse_bwd": ("gsrc",),
           "bn_stats": ("mean", "invstd", "var_unb"), "avgpool": ("y",), "avgpool_bwd": ("gx",)}
EXACT = {"mx", "gx"}        # outputs that are moved or selected, never computed: bound 0 everywhere


def outputs_of(c):
    op = c["op"]
    if op in OUTPUTS:
        return OUTPUTS[op]
    if op == "bn_fwd":
        return ("y", "mean", "invstd") + (("run_mean", "run_var") if c["train"] else ())
    if op == "bn_apply":
        return ("y", "run_mean", "run_var")
    fl = c["flags"]
    return (("dx",) if fl.get("need_dx", True) else ()) + tuple(fl.get("want", ("dgamma", "dbeta")))


def sign_agrees(c, inp, ref):
    """Fraction of ReLU-mask elements whose fp32 forward output (what the backward kernel reads) has another sign than the
    float64 pre-activation: these would have to be left out of the comparison.  Rounding to fp32 keeps the sign, so it is 0."""
    if c["op"] == "hr_fuse_bwd" or (c["op"] == "bn_bwd" and c["relu"]):
        return float(np.mean((inp["y"] > 0) != (ref["pre"] > 0)))
    return 0.0


def shorten(c):
    """A `big` row with few pixels: the same reference path without the second grid-stride trip (for the CPU-only test)."""
    if not c["flags"].get("big"):
        return c
    if "M" in c:
        return dict(c, M=300)
    N, H, W, C = c["shape"]
    return dict(c, shape=(N, 6 + H % 2, 8 + W % 2, C))


def checks(c, ref):
    """[(output name, reference, bound)] of a row, the hr_fuse_bwd list flattened (sources not asked for are left out)."""
    out = []
    for name in outputs_of(c):
        if name == "gsrc":
            out += [(f"gsrc{i}", r, b) for i, (r, b) in enumerate(zip(ref["gsrc"], ref["bounds"]["gsrc"])) if r is not None]
        else:
            out.append((name, ref[name], ref["bounds"][name]))
    return out


def is_exact(c, name):
    """Outputs the kernel moves or selects: their bound is 0 and the comparison bit for bit."""
    if name in EXACT or (name == "mean" and (c["M"] == 1 or not c["train"])):      # eval: the running mean; one pixel: itself
        return True
    if name.startswith("gsrc"):
        return tuple(c["srcs"][int(name[4:])]) == tuple(c["shape"][1:3])
    return False
