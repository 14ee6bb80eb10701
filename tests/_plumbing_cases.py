"""Case tables of tests/test_plumbing_gpu.py: one row per dispatch branch of the trunk / backward / small-shape plumbing
(csrc/trunk_ops.hip, bwd_ops.hip, small_ops.hip), the seeded inputs of each row and its float64 reference on the CPU.

Every row names the KD_NOTE_PLUMBING literal it is meant to reach (`kernel`); tests/test_plumbing_host.py checks, without a
GPU, that every literal in the sources has a row, that every row names a literal the sources declare, and that every row's
reference runs and has the declared shape.  Nothing here touches the device or the library.

Layout: activations are (N, H, W, C) arrays (the kernels' NHWC); `build(case)` returns (inputs, reference) dicts of numpy
arrays: inputs already rounded to the kernel's storage dtype (float32 carriers), references float64.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
U = 2.0 ** -24          # unit roundoff of fp32
OFFSET = 1001.37        # the large common offset one channel of every reduction case carries (spread 1); no round number, so
                        # that a long fp32 chain rounds the same way at every step once its partial sum has grown (a systematic
                        # loss); bf16 stores it as 1000 (multiples of 4 there)


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the bound on a chain of n fp32 roundings."""
    return n * U / (1.0 - n * U)


def q(a, dt):
    """Round to the kernel's storage dtype (round-to-nearest-even), back in a float32 carrier."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DT[dt]).float().numpy()


def rng_of(case):
    return np.random.default_rng(zlib.crc32(case["id"].encode()))


def nchw64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double().permute(0, 3, 1, 2).contiguous()


def nhwc_np(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def offc(C):
    """The channel that carries the large offset."""
    return min(1, C - 1)


CASES = []


def case(op, cid, kernel, **kw):
    c = dict(op=op, id=f"{op}:{cid}", kernel=kernel, **kw)
    CASES.append(c)
    return c


def cases_of(*ops):
    return [c for c in CASES if c["op"] in ops]


def ids(cs):
    return [c["id"] for c in cs]


# =========================================================================================================== kd_channel_sums
def cs_plan(groups, rows, C, vec):
    """kd_channel_sums' launch plan, restated from bwd_ops.hip (cs_chunks and the dispatcher's `chunks` block, and
    channel_sums_partial_kernel's `lc` / `nrl` / `per`): -> dict(chunks, cs_chunks, lc, nrl, per, cblocks, L).
    L is the longest fp32 chain of stage one: a thread adds every nrl-th row of its chunk (ceil(per / nrl) rows), then nrl
    such lane sums are added in LDS in order; stage two is fp64."""
    cs_chunks = min(max((rows + 511) // 512, 1), 1024)
    nvec = (C + 7) // 8 if vec else C
    lc = 32 if nvec > 16 else (16 if nvec > 8 else (8 if nvec > 4 else 4))
    cblocks = (nvec + lc - 1) // lc
    chunks = cs_chunks
    other = groups * cblocks
    want = (2048 + other - 1) // other
    if want < chunks:
        chunks = max(want, 16)
    chunks = min(chunks, cs_chunks)
    nrl = 256 // lc
    per = (rows + chunks - 1) // chunks
    return dict(chunks=chunks, cs_chunks=cs_chunks, lc=lc, nrl=nrl, per=per, cblocks=cblocks, want=want,
                L=(per + nrl - 1) // nrl + nrl)


def _cs(cid, dt, shape, vec=8, sub=False, a=False, per_image=False, sliced=(), **kw):
    return case("channel_sums", f"{cid}-{dt}", f"channel_sums_partial_kernel<{dt},{vec}>", dt=dt, shape=shape, vec=vec, sub=sub, a=a,
                per_image=per_image, sliced=sliced, **kw)


for _dt in ("f32", "bf16"):
    _cs("lc4-one-chunk", _dt, (2, 9, 14, 32), sub=True, a=True, plan=dict(lc=4, chunks=1, cblocks=1))   # the shape the old test had
    _cs("lc8", _dt, (1, 9, 14, 64), a=True, plan=dict(lc=8, chunks=1))                          # nvec = 8
    _cs("lc16", _dt, (1, 9, 14, 128), sub=True, plan=dict(lc=16, chunks=1))                     # nvec = 16
    _cs("lc32", _dt, (1, 9, 14, 256), plan=dict(lc=32, chunks=1, cblocks=1))                    # nvec = 32: one full block
    _cs("two-cblocks", _dt, (1, 9, 14, 512), a=True, plan=dict(lc=32, cblocks=2))               # two channel blocks
    _cs("ragged-cblock", _dt, (1, 9, 14, 264), sub=True, a=True, plan=dict(lc=32, cblocks=2))   # second block holds one vector
    _cs("vec1-C19", _dt, (2, 9, 14, 19), vec=1, sub=True, a=True, plan=dict(lc=32, cblocks=1))  # the logits' channel count
    _cs("vec1-C3", _dt, (2, 9, 14, 3), vec=1, a=True, plan=dict(lc=4))                          # narrower than a block's lanes
    # rows per thread 4 / 5 / 6 / 7 with lc = 4 (64 row lanes, one chunk): the four-row trip leaves 0 / 1 / 2 / 3 rows
    for _rem, _rows in ((0, 256), (1, 320), (2, 384), (3, 448)):
        _cs(f"unroll-rem{_rem}", _dt, (1, 1, _rows, 32), sub=True, a=True, plan=dict(lc=4, chunks=1, nrl=64))
    _cs("unroll-mixed", _dt, (1, 1, 252, 32), plan=dict(lc=4, chunks=1))                        # lanes with 4 and with 3 rows
    # each operand as a channel slice of a wider buffer
    _cs("slice-g", _dt, (2, 5, 7, 32), sub=True, a=True, sliced=("g",))
    _cs("slice-sub", _dt, (2, 5, 7, 32), sub=True, a=True, sliced=("sub",))
    _cs("slice-a", _dt, (2, 5, 7, 32), sub=True, a=True, sliced=("a",))
    _cs("slice-vec1", _dt, (2, 5, 7, 19), vec=1, sub=True, a=True, sliced=("g", "sub", "a"))
    # a misaligned slice of an 8-multiple channel count falls to the scalar kernel
    _cs("misaligned-C32", _dt, (1, 5, 7, 32), vec=1, a=True, sliced=("g",), slice_ld=37, slice_off=3)
# several chunks, ragged last one (70000 rows, 137 chunks of 511, last 504); long enough for the offset channel to bite
_cs("chunks-ragged", "f32", (1, 250, 280, 64), sub=True, a=True, plan=dict(chunks=137, per=511, lc=8), a_near_1=True)
_cs("chunks-ragged", "bf16", (1, 250, 280, 64), sub=True, a=True, plan=dict(chunks=137, per=511, lc=8))
# 16 images x 9 channel blocks = 144 other blocks: want = 15 < 16, the clamp to 16 chunks decides (cs_chunks = 17);
# 8200 rows per image do not divide by 16 (per = 513, last chunk 505)
_cs("want-clamp-16-per-image", "bf16", (16, 82, 100, 265), vec=1, per_image=True, a=True,
    plan=dict(chunks=16, cs_chunks=17, want=15, per=513, cblocks=9))
_cs("per-image-ragged", "f32", (3, 31, 37, 32), per_image=True, sub=True, plan=dict(chunks=3, per=383))   # 1147 rows / 3 chunks
# the 1024-chunk cap: 524800 rows (> 524288), C = 8 (16.8 MB of fp32); per = 513, last chunk ragged
_cs("cap-1024", "f32", (1, 640, 820, 8), a=True, plan=dict(chunks=1024, cs_chunks=1024, per=513, lc=4), ws_bytes=1024 * 2 * 8 * 4,
    bites=True, a_near_1=True)
# the same in bf16, with `sub`: the offset rounds to 1000 (bf16 holds multiples of 4 there) and g - sub carries the low bits
_cs("cap-1024", "bf16", (1, 640, 820, 8), sub=True, a=True, plan=dict(chunks=1024, cs_chunks=1024, per=513, lc=4),
    ws_bytes=1024 * 2 * 8 * 4, a_near_1=True)


def build_channel_sums(c):
    r = rng_of(c)
    N, H, W, C = c["shape"]
    dt = c["dt"]
    g = r.standard_normal(c["shape"])
    g[..., offc(C)] += OFFSET
    inp = {"g": q(g, dt)}
    d = inp["g"].astype(np.float64)
    if c["sub"]:
        inp["sub"] = q(r.standard_normal(c["shape"]) * 0.5, dt)
        d = d - inp["sub"]
    ax = (1, 2) if c["per_image"] else (0, 1, 2)
    ref = {"s1": d.sum(ax), "abs1": np.abs(d).sum(ax)}
    if c["a"]:
        # (long rows: a near 1, so that the products keep the offset and s2 is as exposed to a lossy chain as s1)
        inp["a"] = q(r.standard_normal(c["shape"]) * 0.25 + 1.0 if c.get("a_near_1") else r.standard_normal(c["shape"]) + 0.5, dt)
        ref["s2"] = (d * inp["a"]).sum(ax)
        ref["abs2"] = np.abs(d * inp["a"]).sum(ax)
    return inp, ref


def channel_sums_bound(c, ref, which):
    """|err| <= gamma(L + k) * sum |x_i|: L from cs_plan (stage one's longest fp32 chain), k = 3 operand roundings (g - sub, the
    product with a, the final fp64 -> fp32 store); stage two is fp64 (bwd_ops.hip channel_sums_finish_kernel)."""
    N, H, W, C = c["shape"]
    groups, rows = (N, H * W) if c["per_image"] else (1, N * H * W)
    L = cs_plan(groups, rows, C, c["vec"] == 8)["L"]
    return gamma(L + 3) * ref["abs1" if which == "s1" else "abs2"]


def channel_sums_shape(c):
    N, H, W, C = c["shape"]
    return (N, C) if c["per_image"] else (C,)


# ========================================================================================================= kd_bn_sums_finish
for _rows, _kern in ((1, "channel_sums_finish_kernel"), (256, "channel_sums_finish_kernel"),
                     (257, "bn_sums_stage_kernel<64 rows>"), (1000, "bn_sums_stage_kernel<64 rows>"),      # 1000: ragged 64-row stage
                     (16384, "bn_sums_stage_kernel<64 rows>"), (16385, "bn_sums_stage_kernel<256 rows>")):
    for _C in (8, 24, 256):
        case("bn_sums_finish", f"rows{_rows}-C{_C}", _kern, rows=_rows, C=_C)


def build_bn_sums_finish(c):
    r = rng_of(c)
    part = r.standard_normal((c["rows"], 2, c["C"]))
    part[:, :, offc(c["C"])] += OFFSET
    part = part.astype(np.float32)
    p = part.astype(np.float64)
    return {"part": part}, {"s1": p[:, 0].sum(0), "s2": p[:, 1].sum(0), "abs1": np.abs(p[:, 0]).sum(0), "abs2": np.abs(p[:, 1]).sum(0)}


def bn_sums_finish_bound(c, ref, which):
    """Both stages accumulate in fp64 (bn_sums_stage_kernel, channel_sums_finish_kernel); the fp32 roundings are the stage's
    store (rows > 256 only) and the final store: k = 2 or 1, L = 0; plus the fp64 chain itself."""
    k = 2 if c["rows"] > 256 else 1
    return (gamma(k) + c["rows"] * 2.0 ** -53) * ref["abs1" if which == "s1" else "abs2"]


# ============================================================================================================== elementwise
# kd_relu_bn_bwd: grid_for caps the grid at 16384 blocks of 256 threads, a thread owns 8 channels
for _dt in ("f32", "bf16"):
    case("relu_bn_bwd", f"small-res-{_dt}", f"relu_bn_bwd_kernel<{_dt}>", dt=_dt, shape=(2, 9, 14, 32), res=True, sliced=("mask",))
    case("relu_bn_bwd", f"small-nores-{_dt}", f"relu_bn_bwd_kernel<{_dt}>", dt=_dt, shape=(2, 9, 14, 32), res=False, sliced=("g", "out"))
# 524300 pixels x 8 vectors = 4194400 > 16384 * 256: the grid-stride loop takes a second trip
case("relu_bn_bwd", "grid-stride-bf16", "relu_bn_bwd_kernel<bf16>", dt="bf16", shape=(1, 524, 1001, 64), res=True, sliced=(),
     second_trip=(524 * 1001 * 8, 16384))


def build_relu_bn_bwd(c):
    r = rng_of(c)
    dt, C = c["dt"], c["shape"][3]
    f = lambda s=1.0: q(r.standard_normal(c["shape"], dtype=np.float32) * s, dt)
    inp = {"g": f(), "mask": np.maximum(f(), 0), "scale": (np.abs(r.standard_normal(C)) + 0.5).astype(np.float32)}
    ref = np.where(inp["mask"] > 0, inp["g"].astype(np.float64) * inp["scale"], 0.0)
    if c["res"]:
        inp["res"] = f()
        ref = ref + inp["res"]
    return inp, {"y": ref}


# kd_broadcast_add: same cap
for _dt in ("f32", "bf16"):
    for _acc in (0, 1):
        case("broadcast_add", f"small-acc{_acc}-{_dt}", f"broadcast_add_kernel<{_dt}>", dt=_dt, shape=(2, 5, 7, 32), accumulate=_acc,
             sliced=bool(_acc))
# 2 x 262200 pixels x 8 vectors = 4195200 > 16384 * 256
case("broadcast_add", "grid-stride-acc1-bf16", "broadcast_add_kernel<bf16>", dt="bf16", shape=(2, 437, 600, 64), accumulate=1, sliced=False,
     second_trip=(2 * 437 * 600 * 8, 16384))
case("broadcast_add", "grid-stride-acc0-f32", "broadcast_add_kernel<f32>", dt="f32", shape=(2, 437, 600, 64), accumulate=0, sliced=False,
     second_trip=(2 * 437 * 600 * 8, 16384))


def build_broadcast_add(c):
    r = rng_of(c)
    N, H, W, C = c["shape"]
    v = r.standard_normal((N, C)).astype(np.float32)
    y0 = q(r.standard_normal(c["shape"], dtype=np.float32), c["dt"])
    alpha = 0.5    # a power of two: alpha * v is exact, so accumulate = 0 is a move (bitwise in fp32, one rounding in bf16)
    ref = (y0 if c["accumulate"] else 0.0) + alpha * v.astype(np.float64)[:, None, None, :] + np.zeros(c["shape"])
    return {"v": v, "y0": y0, "alpha": alpha}, {"y": ref}


# ======================================================================================================== kd_aspp_image_pool
def _ip(cid, dt, N, HW, Cin, Cout, sliced=False, **kw):
    return case("aspp_image_pool", f"{cid}-{dt}", f"gap_partial_kernel<{dt}>", dt=dt, N=N, HW=HW, Cin=Cin, Cout=Cout, sliced=sliced, **kw)


_ip("6x10-empty-chunks", "f32", 1, (6, 10), 64, 8)                  # HW = 60 < 64 chunks: four empty ones
_ip("6x10-empty-chunks", "bf16", 3, (6, 10), 64, 8, sliced=True)
_ip("37x41-cin264", "f32", 3, (37, 41), 264, 256, sliced=True)      # two Cin blocks, the second with one octet
_ip("37x41-cin264", "bf16", 1, (37, 41), 264, 8)
_ip("37x41-cin4096", "bf16", 1, (37, 41), 4096, 8)                  # sixteen Cin blocks
# 3 x 32768 pixels x 32 vectors = 3145728 > 8192 * 256: broadcast_kernel's grid-stride loop takes a second trip
_ip("128x256-broadcast-trip", "bf16", 3, (128, 256), 64, 256, second_trip=(3 * 128 * 256 * 32, 8192))
_ip("128x256-cout8", "f32", 1, (128, 256), 64, 8)
# 262144 pixels of 8 channels: long enough for a single fp32 chain over the offset channel to lose bits systematically (its
# partial sums reach 2.6e8, ulp 16 and 32); a thread of gap_partial_kernel adds 512 of them
_ip("512x512-long", "f32", 1, (512, 512), 8, 8)


def build_aspp_image_pool(c):
    r = rng_of(c)
    N, (H, W), Cin, Cout = c["N"], c["HW"], c["Cin"], c["Cout"]
    x = r.standard_normal((N, H, W, Cin), dtype=np.float32)
    x[..., offc(Cin)] += OFFSET
    x = q(x, c["dt"])
    w = (r.standard_normal((Cout, Cin)) * 0.2).astype(np.float32)
    w[:, offc(Cin)] *= 0.05                                  # the offset channel leads the dot product without drowning the others
    sc = (r.standard_normal(Cout) * 0.2 + 1).astype(np.float32)
    sh = (r.standard_normal(Cout) * 0.2).astype(np.float32)
    x64 = x.astype(np.float64).reshape(N, H * W, Cin)
    mean, mabs = x64.mean(1), np.abs(x64).mean(1)
    dot = mean @ w.astype(np.float64).T
    v = np.maximum(dot * sc + sh, 0)
    # error budget of v (relu is 1-Lipschitz): the pooled mean (gap_partial_kernel: a thread adds ceil(per / 8) pixels, 8 lane sums
    # in LDS; gap_finish_kernel: 64 chunk partials in fp32, one division), carried through |w| and |scale|; the dot product
    # (img_conv_kernel: ceil(Cin / 64) fmas per lane, a 6-level wave tree); the scale / shift; the store.
    per = (H * W + 63) // 64
    L1 = (per + 7) // 8 + 8 + 64 + 1
    L2 = (Cin + 63) // 64 + 6 + 1
    bound = np.abs(sc) * ((mabs @ np.abs(w).T.astype(np.float64)) * gamma(L1) + (np.abs(mean) @ np.abs(w).T.astype(np.float64)) * gamma(L2)) \
        + 2 * U * (np.abs(dot * sc) + np.abs(sh))
    if c["dt"] == "bf16":
        bound = bound + 2.0 ** -8 * np.abs(v)          # the bf16 store: 8 significant bits, unit roundoff 2^-8
    return {"x": x, "w": w, "scale": sc, "shift": sh}, {"v": v, "bound": bound, "y": np.broadcast_to(v[:, None, None, :], (N, H, W, Cout))}


# ============================================================================================ kd_maxpool3x3s2 (+ its backward)
POOL_GEOM = [(1, 1), (1, 2), (2, 3), (3, 13), (13, 18), (18, 64), (64, 1), (2, 2), (3, 3), (64, 13)]   # H, W: odd / even mixes
for _dt in ("f32", "bf16"):
    for _H, _W in POOL_GEOM:
        case("maxpool", f"{_H}x{_W}-{_dt}", f"maxpool_kernel<{_dt}>", dt=_dt, shape=(2, _H, _W, 8), outs="both", fill="neg" if _H == 13 else "rand",
             sliced=False)
    case("maxpool", f"raw-only-{_dt}", f"maxpool_kernel<{_dt}>", dt=_dt, shape=(1, 13, 18, 8), outs="raw", fill="rand", sliced=False)
    case("maxpool", f"act-only-{_dt}", f"maxpool_kernel<{_dt}>", dt=_dt, shape=(1, 13, 18, 8), outs="act", fill="rand", sliced=False)
    case("maxpool", f"all-negative-{_dt}", f"maxpool_kernel<{_dt}>", dt=_dt, shape=(1, 3, 2, 8), outs="both", fill="neg", sliced=False)  # 0-padding fails
    case("maxpool", f"C264-slices-{_dt}", f"maxpool_kernel<{_dt}>", dt=_dt, shape=(2, 13, 18, 264), outs="both", fill="neg", sliced=True)


def _pool_x(c, r):
    x = r.standard_normal(c["shape"], dtype=np.float32)
    fill = c["fill"]
    if fill == "neg":
        x = -np.abs(x) - 1.0
    elif fill == "const":
        x[:] = 0.75
    elif fill == "plateau" and c["shape"][1] >= 3 and c["shape"][2] >= 3:
        x[0, :3, :3, :] = x[0, :1, :1, :]           # equal maxima inside and across windows
        x[-1, -3:, -2:, :] = 5.0                     # a plateau that IS the maximum, at the far corner
    return q(x, c["dt"])


def pool_out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def build_maxpool(c):
    r = rng_of(c)
    C = c["shape"][3]
    x = _pool_x(c, r)
    sc = (r.standard_normal(C) * 0.2 + 1).astype(np.float32)
    # (a shift that leaves the ReLU second output a mix of zeros and values, whatever the sign of the input)
    sh = (r.standard_normal(C) * 0.2 + (2.0 if c["fill"] == "neg" else 0.5)).astype(np.float32)
    raw = nhwc_np(F.max_pool2d(nchw64(x), 3, 2, 1))
    return {"x": x, "scale": sc, "shift": sh}, {"raw": raw, "act": np.maximum(raw * sc + sh, 0)}


POOL_BWD_PATHS = {"argmax": "maxpool_argmax_kernel<%s>", "gather8": "maxpool_bwd_kernel<%s,8>", "scalar": "maxpool_bwd_kernel<%s,1>"}
for _dt in ("f32", "bf16"):
    for _path, _lit in POOL_BWD_PATHS.items():
        for _H, _W in POOL_GEOM:
            case("maxpool_bwd", f"{_path}-{_H}x{_W}-{_dt}", _lit % _dt, dt=_dt, path=_path, shape=(2, _H, _W, 8), fill="plateau" if _H >= 3 and _W >= 3 else "rand")
        case("maxpool_bwd", f"{_path}-const-{_dt}", _lit % _dt, dt=_dt, path=_path, shape=(1, 13, 18, 8), fill="const")
        case("maxpool_bwd", f"{_path}-neg-{_dt}", _lit % _dt, dt=_dt, path=_path, shape=(1, 5, 4, 8), fill="neg")
    case("maxpool_bwd", f"scalar-C19-{_dt}", POOL_BWD_PATHS["scalar"] % _dt, dt=_dt, path="dense", shape=(2, 13, 18, 19), fill="plateau")   # C % 8 != 0
    case("maxpool_bwd", f"argmax-C264-{_dt}", POOL_BWD_PATHS["argmax"] % _dt, dt=_dt, path="argmax", shape=(1, 13, 18, 264), fill="plateau")


def build_maxpool_bwd(c):
    r = rng_of(c)
    N, H, W, C = c["shape"]
    x = _pool_x(c, r)
    Ho, Wo = pool_out_hw(H, W)
    gy = q(r.standard_normal((N, Ho, Wo, C), dtype=np.float32), c["dt"])
    xt = nchw64(x).requires_grad_(True)
    F.max_pool2d(xt, 3, 2, 1).backward(nchw64(gy))
    return {"x": x, "gy": gy}, {"gx": nhwc_np(xt.grad)}


# ================================================================================== kd_upsample_bilinear (+ its backward)
# (H, W) -> (Ho, Wo)
UP_SIZES = [((6, 9), (12, 18)),      # x2
            ((5, 7), (20, 28)),      # x4
            ((7, 10), (18, 23)),     # non-integer ratio up
            ((7, 10), (7, 10)),      # identity
            ((32, 48), (4, 6)),      # down-sampling by 8 (the forward whose adjoint engine.py's edge path takes)
            ((18, 23), (7, 10)),     # non-integer ratio down
            ((5, 7), (1, 9)),        # Ho == 1
            ((5, 7), (9, 1)),        # Wo == 1
            ((1, 7), (4, 14))]       # H == 1
# the flat kernel needs Wo * C % 4 == 0 with C % 8 != 0 and a dense fp32 output
UP_SIZES_FLAT4 = [((6, 9), (12, 20)), ((5, 7), (20, 28)), ((7, 10), (18, 24)), ((7, 12), (7, 12)), ((32, 48), (4, 8)), ((18, 23), (7, 12)),
                  ((5, 7), (1, 12)), ((1, 7), (4, 16))]
_DN = {"f32": "f32", "bf16": "bf16"}


def _sz(a, b):
    return f"{a[0]}x{a[1]}to{b[0]}x{b[1]}"


for _al in (True, False):
    _m = "ac" if _al else "nac"
    for _ti in ("f32", "bf16"):
        for _to in ("f32", "bf16"):
            for _hin, _hout in UP_SIZES:
                case("upsample", f"v8-{_ti}-{_to}-{_m}-{_sz(_hin, _hout)}", f"upsample_kernel<{_ti},{_to},8>", ti=_ti, to=_to, align=_al, C=8,
                     hin=_hin, hout=_hout, sliced=False, N=2)
                # C = 19 into a slice of a wider buffer, as the engine writes the logits of GSCNN's heads; also what keeps a dense
                # fp32 output from taking the flat kernel
                case("upsample", f"v1-{_ti}-{_to}-{_m}-{_sz(_hin, _hout)}", f"upsample_kernel<{_ti},{_to},1>", ti=_ti, to=_to, align=_al, C=19,
                     hin=_hin, hout=_hout, sliced=True, N=2)
            case("upsample", f"v8-C256-slice-{_ti}-{_to}-{_m}", f"upsample_kernel<{_ti},{_to},8>", ti=_ti, to=_to, align=_al, C=256, hin=(7, 10),
                 hout=(18, 23), sliced=True, N=1)
            case("upsample", f"v1-C1-{_ti}-{_to}-{_m}", f"upsample_kernel<{_ti},{_to},1>", ti=_ti, to=_to, align=_al, C=1, hin=(7, 10),
                 hout=(18, 23), sliced=_to == "f32", N=2)
        for _hin, _hout in UP_SIZES_FLAT4:
            case("upsample", f"flat4-{_ti}-{_m}-{_sz(_hin, _hout)}", f"upsample_flat4_kernel<{_ti}>", ti=_ti, to="f32", align=_al, C=19, hin=_hin,
                 hout=_hout, sliced=False, N=2)
        case("upsample", f"flat4-C1-{_ti}-{_m}", f"upsample_flat4_kernel<{_ti}>", ti=_ti, to="f32", align=_al, C=1, hin=(7, 10), hout=(18, 24),
             sliced=False, N=2)
        # several 256-thread blocks per output row, ragged last one (668 * 19 / 4 = 3173 threads)
        case("upsample", f"flat4-wide-{_ti}-{_m}", f"upsample_flat4_kernel<{_ti}>", ti=_ti, to="f32", align=_al, C=19, hin=(21, 333), hout=(42, 668),
             sliced=False, N=1)
    # backward: <gy dtype, gx dtype, VEC>
    for _tg in ("f32", "bf16"):
        for _tx in ("f32", "bf16"):
            for _hin, _hout in UP_SIZES:
                case("upsample_bwd", f"v8-{_tg}-{_tx}-{_m}-{_sz(_hin, _hout)}", f"upsample_bwd_kernel<{_tg},{_tx},8>", tg=_tg, tx=_tx, align=_al,
                     C=8, hin=_hin, hout=_hout, sliced=False, N=2)
                case("upsample_bwd", f"v1-{_tg}-{_tx}-{_m}-{_sz(_hin, _hout)}", f"upsample_bwd_kernel<{_tg},{_tx},1>", tg=_tg, tx=_tx, align=_al,
                     C=19, hin=_hin, hout=_hout, sliced=True, N=2)      # gx: a C = 19 slice of a wider buffer
            case("upsample_bwd", f"v8-C256-{_tg}-{_tx}-{_m}", f"upsample_bwd_kernel<{_tg},{_tx},8>", tg=_tg, tx=_tx, align=_al, C=256,
                 hin=(7, 10), hout=(18, 23), sliced=True, N=1)
            case("upsample_bwd", f"v1-C1-{_tg}-{_tx}-{_m}", f"upsample_bwd_kernel<{_tg},{_tx},1>", tg=_tg, tx=_tx, align=_al, C=1,
                 hin=(32, 48), hout=(4, 6), sliced=False, N=2)         # the one-channel edge gradient, adjoint of a down-sampling


def build_upsample(c):
    r = rng_of(c)
    x = q(r.standard_normal((c["N"],) + c["hin"] + (c["C"],), dtype=np.float32), c["ti"])
    y = F.interpolate(nchw64(x), size=c["hout"], mode="bilinear", align_corners=c["align"])
    return {"x": x}, {"y": nhwc_np(y)}


def build_upsample_bwd(c):
    r = rng_of(c)
    gy = q(r.standard_normal((c["N"],) + c["hout"] + (c["C"],), dtype=np.float32), c["tg"])
    xi = torch.zeros((c["N"], c["C"]) + c["hin"], dtype=torch.float64, requires_grad=True)
    F.interpolate(xi, size=c["hout"], mode="bilinear", align_corners=c["align"]).backward(nchw64(gy))
    return {"gy": gy}, {"gx": nhwc_np(xi.grad)}


# ============================================================================================================ kd_zero_insert
for _dt in ("f32", "bf16"):
    for _s, _extra in ((1, (0, 0)), (2, (0, 0)), (2, (1, 1)), (3, (0, 0)), (3, (2, 1))):     # Hy, Wy at and above the minimum
        case("zero_insert", f"s{_s}-extra{_extra[0]}{_extra[1]}-{_dt}", f"zero_insert_kernel<{_dt}>", dt=_dt, shape=(2, 5, 7, 16), stride=_s,
             extra=_extra)


def build_zero_insert(c):
    r = rng_of(c)
    N, H, W, C = c["shape"]
    s = c["stride"]
    x = q(r.standard_normal(c["shape"], dtype=np.float32), c["dt"])
    Hy, Wy = (H - 1) * s + 1 + c["extra"][0], (W - 1) * s + 1 + c["extra"][1]
    y = torch.zeros((N, Hy, Wy, C), dtype=torch.float64)
    y[:, :(H - 1) * s + 1:s, :(W - 1) * s + 1:s] = torch.from_numpy(x).double()
    return {"x": x, "size": (Hy, Wy)}, {"y": y.numpy()}


# ============================================================================================================== kd_copy_cast
# layouts of (src, dst): "nchw" dense NCHW, "cl" channels_last, "cl_slice" a channel slice of a wider channels_last buffer
for _sd in ("f32", "bf16"):
    for _dd in ("f32", "bf16"):
        case("copy_cast", f"nchw-to-cl-{_sd}-{_dd}", "copy_cast_kernel<c_fast>", sd=_sd, dd=_dd, src="nchw", dst="cl", shape=(2, 19, 5, 7))
        case("copy_cast", f"clslice-to-nchw-{_sd}-{_dd}", "copy_cast_kernel<p_fast>", sd=_sd, dd=_dd, src="cl_slice", dst="nchw", shape=(2, 19, 5, 7))
        case("copy_cast", f"nchw-to-nchw-{_sd}-{_dd}", "copy_cast_kernel<p_fast>", sd=_sd, dd=_dd, src="nchw", dst="nchw", shape=(2, 19, 5, 7))
        case("copy_cast", f"cl-to-clslice-{_sd}-{_dd}", "copy_cast_kernel<c_fast>", sd=_sd, dd=_dd, src="cl", dst="cl_slice", shape=(2, 19, 5, 7))
# 16 x (2^24 + 5) = 2^28 + 80 elements > 2^20 blocks x 256 threads: the grid-stride loop takes a second trip (0.5 GB each side)
case("copy_cast", "grid-stride-bf16", "copy_cast_kernel<c_fast>", sd="bf16", dd="bf16", src="nchw", dst="cl", shape=(1, 16, 1, (1 << 24) + 5),
     second_trip=(16 * ((1 << 24) + 5), 1 << 20), big=True)


def build_copy_cast(c):
    """Logical NCHW arrays.  Values keep more bits than bf16 holds, so an fp32 -> bf16 case rounds (nearest even)."""
    r = rng_of(c)
    shape = c["shape"]
    n = int(np.prod(shape))
    if c.get("big"):
        base = torch.from_numpy(r.standard_normal(1000003, dtype=np.float32))     # a prime period: a misplaced element shows
        src = base.repeat(n // 1000003 + 1)[:n].reshape(shape)
    else:
        src = torch.from_numpy(r.standard_normal(shape, dtype=np.float32))
        src.view(-1)[::7] = torch.tensor(1.00390625)                                # 1 + 2^-8: a tie in bf16 (rounds to even, 1.0)
    src = src.to(DT[c["sd"]])
    return {"src": src}, {"dst": src.to(DT[c["dd"]])}      # torch tensors here: the comparison is bitwise, in the storage dtype


# ================================================================================================= kd_bn_fold / param grads
for _C in (8, 600):     # 600: three 256-thread blocks, the last ragged
    case("bn_fold", f"C{_C}", "bn_fold_kernel", C=_C)
    for _acc in (0, 1):
        case("bn_eval_param_grads", f"C{_C}-acc{_acc}", "bn_eval_param_grads_kernel", C=_C, accumulate=_acc)


def build_bn_fold(c):
    r = rng_of(c)
    C = c["C"]
    f = lambda: r.standard_normal(C).astype(np.float32)
    g, b, m, v = f(), f(), f(), (np.abs(f()) + 0.1).astype(np.float32)
    g[3] = 0.0                                              # a channel with gamma = 0: scale 0, shift = beta
    eps = 1e-5
    sc = g.astype(np.float64) / np.sqrt(v.astype(np.float64) + eps)
    return {"gamma": g, "beta": b, "mean": m, "var": v, "eps": eps}, {"scale": sc, "shift": b - m * sc}


def build_bn_eval_param_grads(c):
    r = rng_of(c)
    C = c["C"]
    f = lambda: r.standard_normal(C).astype(np.float32)
    s1, s2, g, b, v = f() * 10, f() * 10, f(), f(), (np.abs(f()) + 0.1).astype(np.float32)
    g[3] = 0.0                                              # gamma = 0 (hence scale = 0): both gradients are 0
    sc = (g / np.sqrt(v + 1e-5)).astype(np.float32)
    s1d, s2d, scd, gd, bd = (t.astype(np.float64) for t in (s1, s2, sc, g, b))
    ok = (scd != 0) & (gd != 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        db = np.where(scd != 0, s1d / scd, 0.0)
        dg = np.where(ok, (s2d - bd * s1d) / (scd * gd), 0.0)
    return {"s1": s1, "s2": s2, "scale": sc, "gamma": g, "beta": b}, {"dgamma": dg, "dbeta": db}


# ================================================================================================ kd_stem_conv / kd_stem_wgrad
case("stem_conv", "H1-N3-f32", "stem_conv_kernel<f32>", dt="f32", shape=(3, 1, 21))               # H = 1, W % 16 != 0, N = 3
case("stem_conv", "H1-N3-bf16", "stem_conv_mfma_kernel", dt="bf16", shape=(3, 1, 21))
case("stem_conv", "5x33-f32", "stem_conv_kernel<f32>", dt="f32", shape=(1, 5, 33))
case("stem_conv", "5x33-bf16", "stem_conv_mfma_kernel", dt="bf16", shape=(1, 5, 33))
# 129 rows x 128 groups of 16 columns = 16512 row groups > the 4096-block x 4-wave persistent grid: a second trip
case("stem_conv", "persistent-bf16", "stem_conv_mfma_kernel", dt="bf16", shape=(1, 129, 2041), second_trip=(129 * 128, 64))
case("stem_conv_pool", "20x28", "stem_pool_kernel", shape=(2, 20, 28))
case("stem_conv_pool", "17x37", "stem_pool_kernel", shape=(1, 17, 37))                            # odd sizes, ragged column group


def _stem_xw(c, r, dt):
    N, H, W = c["shape"]
    x = r.standard_normal((N, 3, H, W), dtype=np.float32)
    w = (r.standard_normal((64, 3, 3, 3)) * 0.2).astype(np.float32)
    return x, w


def build_stem_conv(c):
    r = rng_of(c)
    x, w = _stem_xw(c, r, c["dt"])
    # the bf16 kernel rounds the image and the weight to bf16 for the matrix cores; the fp32 one keeps both
    y = F.conv2d(torch.from_numpy(q(x, c["dt"])).double(), torch.from_numpy(q(w, c["dt"])).double(), padding=1)
    return {"x": x, "w": w}, {"y": nhwc_np(y)}


def build_stem_conv_pool(c):
    r = rng_of(c)
    x, w = _stem_xw(c, r, "bf16")
    y = F.conv2d(torch.from_numpy(q(x, "bf16")).double(), torch.from_numpy(q(w, "bf16")).double(), padding=1)
    raw = nhwc_np(F.max_pool2d(y, 3, 2, 1))
    sc = (r.standard_normal(64) * 0.2 + 1).astype(np.float32)
    sh = (r.standard_normal(64) * 0.2).astype(np.float32)
    return {"x": x, "w": w, "scale": sc, "shift": sh}, {"raw": raw, "act": np.maximum(raw * sc + sh, 0)}


# dy views: "dense" ld 64; "ld72" / "ld68": a 64-channel slice at element 8 / 4 of a 72 / 68-wide buffer; "off1": at element 1
# of a 72-wide buffer (2-byte offset: not 16-B aligned)
for _cid, _kern, _dt, _view, _shape in (
        ("mfma-dense", "stem_wgrad_mfma_kernel", "bf16", "dense", (2, 11, 270)),       # 44 work items (< 768), two column segments
        ("mfma-ld72", "stem_wgrad_mfma_kernel", "bf16", "ld72", (2, 11, 270)),         # ld % 8 == 0 stays on the matrix cores
        ("valu-ld68", "stem_wgrad_kernel<bf16>", "bf16", "ld68", (2, 11, 270)),        # ld % 8 != 0
        ("valu-off1", "stem_wgrad_kernel<bf16>", "bf16", "off1", (3, 1, 21)),          # unaligned view; H = 1, N = 3
        ("f32-dense", "stem_wgrad_kernel<f32>", "f32", "dense", (2, 11, 270)),
        ("mfma-800-items", "stem_wgrad_mfma_kernel", "bf16", "dense", (2, 400, 16)),   # 800 work items > 768 blocks: a second trip
        ("valu-800-items", "stem_wgrad_kernel<bf16>", "bf16", "ld68", (2, 400, 16)),
        ("f32-800-items", "stem_wgrad_kernel<f32>", "f32", "dense", (2, 400, 16))):
    case("stem_wgrad", _cid, _kern, dt=_dt, view=_view, shape=_shape)


def build_stem_wgrad(c):
    r = rng_of(c)
    N, H, W = c["shape"]
    x = r.standard_normal((N, 3, H, W), dtype=np.float32)
    x[:, 1] += 30.0                                  # an image plane with a common offset (pixel values are not centred)
    dy = q(r.standard_normal((N, H, W, 64), dtype=np.float32), c["dt"])
    xt, gt = torch.from_numpy(x).double(), nchw64(dy)

    def wgrad(a, g):
        w = torch.zeros((64, 3, 3, 3), dtype=torch.float64, requires_grad=True)
        F.conv2d(a, w, padding=1).backward(g)
        return w.grad.numpy()
    return {"x": x, "dy": dy}, {"dw": wgrad(xt, gt), "abs": wgrad(xt.abs(), gt.abs())}


def stem_wgrad_bound(c, ref):
    """gamma(L + k) * sum |dy x|: a block walks ceil(items / blocks) work items (stem_blocks: at most 768 blocks) of up to 256
    pixels; the VALU kernel's thread adds every 4th pixel of an item, four phase sums follow (stem_wgrad_kernel); the MFMA kernel
    contracts all 256 (zero-padded) pixels of an item into one accumulator (stem_wgrad_mfma_kernel); blocks are added in fp64
    (stem_wgrad_finish_kernel).  k = 2: the product and the final store."""
    N, H, W = c["shape"]
    items = N * H * ((W + 255) // 256)
    per_block = (items + min(items, 768) - 1) // min(items, 768)
    L = per_block * 256 if "mfma" in c["kernel"] else per_block * ((min(W, 256) + 3) // 4) + 3
    return gamma(L + 2) * ref["abs"]


# =================================================================================== kd_bn2d_fwd / bwd, kd_conv2d_direct_wgrad
CIFAR = [(128, 16, 32, 32), (128, 32, 16, 16), (128, 64, 8, 8)]        # the shapes the ResNet-20 / WRN small-shape path runs
for _N, _C, _H, _W in CIFAR:
    for _train in (True, False):
        for _relu in (True, False):
            _t = "train" if _train else "eval"
            case("bn2d_fwd", f"C{_C}-{_t}-relu{int(_relu)}", f"bn2d_fwd_kernel<{_t}>", shape=(_N, _C, _H, _W), train=_train, relu=_relu)
            case("bn2d_bwd", f"C{_C}-{_t}-relu{int(_relu)}", f"bn2d_bwd_kernel<{_t}>", shape=(_N, _C, _H, _W), train=_train, relu=_relu,
                 need_dx=True)
    case("bn2d_bwd", f"C{_C}-train-nodx", "bn2d_bwd_kernel<train>", shape=(_N, _C, _H, _W), train=True, relu=True, need_dx=False)
case("bn2d_fwd", "odd-small", "bn2d_fwd_kernel<train>", shape=(3, 5, 7, 9), train=True, relu=True)      # M = 189 < one block's threads
case("bn2d_bwd", "odd-small", "bn2d_bwd_kernel<train>", shape=(3, 5, 7, 9), train=True, relu=True, need_dx=True)
BN_EPS, BN_MOM = 1e-5, 0.1


def _bn_inputs(c, r):
    N, C, H, W = c["shape"]
    x = r.standard_normal(c["shape"], dtype=np.float32)
    x[:, offc(C)] += OFFSET
    g = (r.standard_normal(C) * 0.3 + 1).astype(np.float32)
    b = (r.standard_normal(C) * 0.3).astype(np.float32)
    rm = (r.standard_normal(C) * 0.1).astype(np.float32)
    rm[offc(C)] += OFFSET
    rv = (np.abs(r.standard_normal(C)) + 0.5).astype(np.float32)
    return x, g, b, rm, rv


def bn_chain(M):
    """bn2d_*_kernel: a thread adds every 256th of the channel's M values, block_sum256 follows (6 shuffles, 2 adds)."""
    return (M + 255) // 256 + 8


def build_bn2d_fwd(c):
    r = rng_of(c)
    N, C, H, W = c["shape"]
    x, g, b, rm, rv = _bn_inputs(c, r)
    M = N * H * W
    x64 = torch.from_numpy(x).double()
    rm64, rv64 = torch.from_numpy(rm).double(), torch.from_numpy(rv).double()
    y = F.batch_norm(x64, rm64, rv64, torch.from_numpy(g).double(), torch.from_numpy(b).double(), c["train"], BN_MOM, BN_EPS)  # updates rm64 / rv64
    if c["relu"]:
        y = torch.relu(y)
    xc = x64.transpose(0, 1).reshape(C, -1)
    mean = xc.mean(1) if c["train"] else torch.from_numpy(rm).double()
    var = xc.var(1, unbiased=False) if c["train"] else torch.from_numpy(rv).double()
    ref = {"y": y.numpy(), "mean": mean.numpy(), "invstd": (1 / torch.sqrt(var + BN_EPS)).numpy(), "run_mean": rm64.numpy(), "run_var": rv64.numpy(),
           "absmean": xc.abs().mean(1).numpy(), "var": var.numpy()}
    return {"x": x, "gamma": g, "beta": b, "run_mean": rm, "run_var": rv}, ref


def build_bn2d_bwd(c):
    r = rng_of(c)
    N, C, H, W = c["shape"]
    x, g, b, rm, rv = _bn_inputs(c, r)
    dy = r.standard_normal(c["shape"], dtype=np.float32)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    g64, b64 = torch.from_numpy(g).double().requires_grad_(True), torch.from_numpy(b).double().requires_grad_(True)
    y = F.batch_norm(x64, torch.from_numpy(rm).double(), torch.from_numpy(rv).double(), g64, b64, c["train"], BN_MOM, BN_EPS)
    if c["relu"]:
        y = torch.relu(y)
    y.backward(torch.from_numpy(dy).double())
    xc = x64.detach().transpose(0, 1).reshape(C, -1)
    mean = xc.mean(1) if c["train"] else torch.from_numpy(rm).double()
    var = xc.var(1, unbiased=False) if c["train"] else torch.from_numpy(rv).double()
    invstd = 1 / torch.sqrt(var + BN_EPS)
    # the saved statistics and the forward output the kernel is handed: the reference's, rounded to fp32
    mean32, is32, y32 = mean.float().numpy(), invstd.float().numpy(), y.detach().float().numpy()
    gm = torch.from_numpy(dy).double() * ((y.detach() > 0) if c["relu"] else 1.0)
    xhat = (x64.detach() - mean[None, :, None, None]) * invstd[None, :, None, None]
    ref = {"dx": x64.grad.numpy(), "dgamma": g64.grad.numpy(), "dbeta": b64.grad.numpy(),
           "abs_g": gm.abs().sum((0, 2, 3)).numpy(), "abs_gx": (gm * xhat).abs().sum((0, 2, 3)).numpy(),
           "mean": mean.numpy(), "invstd": invstd.numpy()}
    return {"dy": dy, "x": x, "y": y32, "gamma": g, "mean": mean32, "invstd": is32}, ref


def bn2d_bwd_bounds(c, ref):
    """dbeta: gamma(L + 1) sum |g|.  dgamma = sum g * (x - mean) * invstd: gamma(L + 4) sum |g xhat| (subtraction, two products,
    the store), plus what the fp32 rounding of the saved mean moves it by: u |mean| invstd sum |g|."""
    N, C, H, W = c["shape"]
    L = bn_chain(N * H * W)
    return (gamma(L + 4) * ref["abs_gx"] + U * np.abs(ref["mean"]) * ref["invstd"] * ref["abs_g"], gamma(L + 1) * ref["abs_g"])


# N, C, H, W, K, k, stride, pad, groups, bias
for _cid, _d in (("stem-3to16", (128, 3, 32, 32, 16, 3, 1, 1, 1, False)),
                 ("16to16-32x32", (128, 16, 32, 32, 16, 3, 1, 1, 1, True)),
                 ("16to32-s2", (128, 16, 32, 32, 32, 3, 2, 1, 1, False)),
                 ("32to64-1x1-s2", (128, 32, 16, 16, 64, 1, 2, 0, 1, True)),
                 ("64-depthwise-8x8", (128, 64, 8, 8, 64, 3, 1, 1, 64, True))):
    case("direct_wgrad", _cid, "dconv_wgrad_kernel", desc=_d)


def build_direct_wgrad(c):
    r = rng_of(c)
    N, C, H, W, K, k, s, p, g, has_b = c["desc"]
    x = r.standard_normal((N, C, H, W), dtype=np.float32)
    x[:, offc(C)] += 30.0
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = r.standard_normal((N, K, Ho, Wo), dtype=np.float32)

    def wgrad(a, gg):
        w = torch.zeros((K, C // g, k, k), dtype=torch.float64, requires_grad=True)
        F.conv2d(a, w, stride=s, padding=p, groups=g).backward(gg)
        return w.grad.numpy()
    xt, gt = torch.from_numpy(x).double(), torch.from_numpy(dy).double()
    ref = {"dw": wgrad(xt, gt), "abs_w": wgrad(xt.abs(), gt.abs()), "db": gt.sum((0, 2, 3)).numpy(), "abs_b": gt.abs().sum((0, 2, 3)).numpy()}
    return {"x": x, "dy": dy}, ref


def direct_wgrad_bounds(c, ref):
    """dconv_wgrad_kernel / dconv_bias_grad_kernel: a thread adds every 256th of the N * Ho * Wo pixels (fma: one rounding per
    term), block_sum256 follows; k = 1 for the store."""
    N, C, H, W, K, k, s, p, g, has_b = c["desc"]
    npix = N * ((H + 2 * p - k) // s + 1) * ((W + 2 * p - k) // s + 1)
    L = bn_chain(npix)
    return gamma(L + 1) * ref["abs_w"], gamma(L + 1) * ref["abs_b"]


BUILDERS = {"channel_sums": build_channel_sums, "bn_sums_finish": build_bn_sums_finish, "relu_bn_bwd": build_relu_bn_bwd,
            "broadcast_add": build_broadcast_add, "aspp_image_pool": build_aspp_image_pool, "maxpool": build_maxpool,
            "maxpool_bwd": build_maxpool_bwd, "upsample": build_upsample, "upsample_bwd": build_upsample_bwd, "zero_insert": build_zero_insert,
            "copy_cast": build_copy_cast, "bn_fold": build_bn_fold, "bn_eval_param_grads": build_bn_eval_param_grads,
            "stem_conv": build_stem_conv, "stem_conv_pool": build_stem_conv_pool, "stem_wgrad": build_stem_wgrad, "bn2d_fwd": build_bn2d_fwd,
            "bn2d_bwd": build_bn2d_bwd, "direct_wgrad": build_direct_wgrad}


def build(c):
    return BUILDERS[c["op"]](c)


def expected_shapes(c):
    """{reference name: shape} each case declares, from its parameters alone (test_plumbing_host.py holds build() to it)."""
    op = c["op"]
    if op == "channel_sums":
        s = channel_sums_shape(c)
        return {"s1": s, **({"s2": s} if c["a"] else {})}
    if op == "bn_sums_finish":
        return {"s1": (c["C"],), "s2": (c["C"],)}
    if op in ("relu_bn_bwd", "broadcast_add"):
        return {"y": c["shape"]}
    if op == "aspp_image_pool":
        return {"y": (c["N"],) + c["HW"] + (c["Cout"],), "v": (c["N"], c["Cout"]), "bound": (c["N"], c["Cout"])}
    if op == "maxpool":
        N, H, W, C = c["shape"]
        o = (N,) + pool_out_hw(H, W) + (C,)
        return {"raw": o, "act": o}
    if op == "maxpool_bwd":
        return {"gx": c["shape"]}
    if op == "upsample":
        return {"y": (c["N"],) + c["hout"] + (c["C"],)}
    if op == "upsample_bwd":
        return {"gx": (c["N"],) + c["hin"] + (c["C"],)}
    if op == "zero_insert":
        N, H, W, C = c["shape"]
        s = c["stride"]
        return {"y": (N, (H - 1) * s + 1 + c["extra"][0], (W - 1) * s + 1 + c["extra"][1], C)}
    if op == "copy_cast":
        return {"dst": c["shape"]}
    if op == "bn_fold":
        return {"scale": (c["C"],), "shift": (c["C"],)}
    if op == "bn_eval_param_grads":
        return {"dgamma": (c["C"],), "dbeta": (c["C"],)}
    if op == "stem_conv":
        N, H, W = c["shape"]
        return {"y": (N, H, W, 64)}
    if op == "stem_conv_pool":
        N, H, W = c["shape"]
        o = (N,) + pool_out_hw(H, W) + (64,)
        return {"raw": o, "act": o}
    if op == "stem_wgrad":
        return {"dw": (64, 3, 3, 3)}
    if op == "bn2d_fwd":
        C = c["shape"][1]
        return {"y": c["shape"], "mean": (C,), "invstd": (C,), "run_mean": (C,), "run_var": (C,)}
    if op == "bn2d_bwd":
        C = c["shape"][1]
        return {"dx": c["shape"], "dgamma": (C,), "dbeta": (C,)}
    if op == "direct_wgrad":
        N, C, H, W, K, k, s, p, g, has_b = c["desc"]
        return {"dw": (K, C // g, k, k), "db": (K,)}
    raise KeyError(op)


# ============================================================================= what a single fp32 chain would do to each reduction
REDUCTIONS = ("channel_sums", "bn_sums_finish", "aspp_image_pool", "bn2d_fwd", "bn2d_bwd", "stem_wgrad", "direct_wgrad")


def chain32(terms):
    """Sequential fp32 accumulation of `terms` (rounded to fp32 first), in order."""
    return float(np.cumsum(np.asarray(terms, dtype=np.float32).ravel(), dtype=np.float32)[-1])


def single_chain(c, inp, ref):
    """{quantity: (error of ONE fp32 chain over the same data, the bound the kernel's decomposition is held to)} for the element of
    each reduced quantity that the large offset reaches.  Operands are formed in fp32, as the kernel forms them."""
    op = c["op"]
    out = {}
    if op == "channel_sums":
        C = c["shape"][3]
        ch = offc(C)
        rows = (lambda t: t[0].reshape(-1, C)[:, ch]) if c["per_image"] else (lambda t: t.reshape(-1, C)[:, ch])
        d = rows(inp["g"]).astype(np.float32)
        if c["sub"]:
            d = d - rows(inp["sub"])
        pick = (lambda v: v[0, ch]) if c["per_image"] else (lambda v: v[ch])
        out["s1"] = (abs(chain32(d) - pick(ref["s1"])), pick(channel_sums_bound(c, ref, "s1")))
        if c["a"]:
            out["s2"] = (abs(chain32(d * rows(inp["a"])) - pick(ref["s2"])), pick(channel_sums_bound(c, ref, "s2")))
    elif op == "bn_sums_finish":
        ch = offc(c["C"])
        for i, k in enumerate(("s1", "s2")):
            out[k] = (abs(chain32(inp["part"][:, i, ch]) - ref[k][ch]), bn_sums_finish_bound(c, ref, k)[ch])
    elif op == "aspp_image_pool":
        # the pooled mean of image 0 by one chain per channel, then the float64 dot / scale / shift / relu of the reference
        x = inp["x"][0].reshape(-1, c["Cin"])
        mean = np.cumsum(x, axis=0, dtype=np.float32)[-1].astype(np.float64) / x.shape[0]
        v = np.maximum((mean @ inp["w"].astype(np.float64).T) * inp["scale"] + inp["shift"], 0)
        err = np.abs(v - ref["v"][0])
        j = int(np.argmax(err / ref["bound"][0]))
        out["v"] = (err[j], ref["bound"][0][j])
    elif op == "bn2d_fwd":
        if c["train"]:
            N, C, H, W = c["shape"]
            ch = offc(C)
            bm = gamma(bn_chain(N * H * W) + 2) * ref["absmean"][ch]
            out["mean"] = (abs(chain32(inp["x"][:, ch]) / (N * H * W) - ref["mean"][ch]), bm)
    elif op == "bn2d_bwd":
        ch = offc(c["shape"][1])
        g = inp["dy"][:, ch] * ((inp["y"][:, ch] > 0) if c["relu"] else 1.0)
        xhat = (inp["x"][:, ch] - inp["mean"][ch]) * inp["invstd"][ch]
        bg, bb = bn2d_bwd_bounds(c, ref)
        out["dbeta"] = (abs(chain32(g) - ref["dbeta"][ch]), bb[ch])
        out["dgamma"] = (abs(chain32(g.astype(np.float32) * xhat.astype(np.float32)) - ref["dgamma"][ch]), bg[ch])
    elif op == "stem_wgrad":
        # the centre tap of (output channel 0, the image plane with the offset): dy and x meet at the same pixel
        terms = inp["dy"][..., 0] * inp["x"][:, 1]
        out["dw"] = (abs(chain32(terms) - ref["dw"][0, 1, 1, 1]), stem_wgrad_bound(c, ref)[0, 1, 1, 1])
    elif op == "direct_wgrad":
        N, C, H, W, K, k, s, p, g, has_b = c["desc"]
        bw, bb = direct_wgrad_bounds(c, ref)
        out["db"] = (abs(chain32(inp["dy"][:, offc(K)]) - ref["db"][offc(K)]), bb[offc(K)])
    return out


# ---- the role of every reduction row in that respect (tests/test_plumbing_host.py asserts it on the CPU) -------------------
#   chain = ("bites", quantities): ONE fp32 chain over the row's data misses the bound for these quantities, so the row fails a
#           kernel whose decomposition loses the low bits;
#   chain = ("inside", why): a single chain stays inside the bound (asserted as well): the row checks indexing, not precision;
#   chain = ("marginal", why): a single chain's error is of the order of the bound and decides nothing either way.
SHORT = "a few hundred rows at most per sum: a single chain is no longer than the kernel's own stage-one chain"
ZERO_MEAN = "the summed products have no common sign (the gradient is zero-mean): a chain's roundings do not add up"
for _c in CASES:
    _op = _c["op"]
    if _op == "channel_sums":
        _long = {"channel_sums:chunks-ragged-f32": ("s1",),        # 70000 rows; s2's error is of the order of its bound
                 "channel_sums:cap-1024-f32": ("s1", "s2"),        # 524800 rows
                 "channel_sums:cap-1024-bf16": ("s1", "s2")}       # the same in bf16: g - sub carries the low bits
        if _c["id"] in _long:
            _c["chain"] = ("bites", _long[_c["id"]])
        elif _c["id"] == "channel_sums:chunks-ragged-bf16":
            _c["chain"] = ("inside", "70000 rows of bf16 data at the offset: partial sums reach 7e7 (ulp 4 to 8, the grid the data lie on)")
        elif _c["id"] == "channel_sums:want-clamp-16-per-image-bf16":
            _c["chain"] = ("inside", "8200 rows per image of multiples of 4: fp32 adds them exactly")
        else:
            _c["chain"] = ("inside", SHORT)
    elif _op == "bn_sums_finish":
        # the kernel accumulates in fp64 and is held to two fp32 roundings: 16384 rows in fp32 must miss that
        _c["chain"] = ("bites", ("s1", "s2")) if _c["rows"] >= 16384 else \
            (("inside", "one row: nothing to add") if _c["rows"] == 1 else
             ("marginal", "256 to 1000 rows: an fp32 chain errs by one to five times the two-rounding bound, channel by channel"))
    elif _op == "aspp_image_pool":
        _c["chain"] = ("bites", ("v",)) if _c["id"] == "aspp_image_pool:512x512-long-f32" else \
            ("inside", "at most 32768 pixels per image: partial sums stay below 2^25, where fp32's ulp is no larger than the spread (and exact for bf16)")
    elif _op == "bn2d_fwd":
        if _c["train"]:
            # 131072 values per channel at 32x32; 32768 / 8192 at 16x16 / 8x8, where the kernel's own per-thread chain (128 / 32
            # terms + 8) is within reach of what a single chain loses
            _c["chain"] = ("bites", ("mean",)) if _c["shape"] == (128, 16, 32, 32) else \
                ("inside", "at most 32768 values per channel: partial sums stay below 2^25, ulp no larger than the spread")
        else:
            _c["chain"] = ("inside", "eval mode reduces nothing")
    elif _op in ("bn2d_bwd", "stem_wgrad", "direct_wgrad"):
        _c["chain"] = ("inside", ZERO_MEAN)
