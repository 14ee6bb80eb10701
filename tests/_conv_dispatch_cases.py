"""Case table of tests/test_conv_dispatch_gpu.py: one row per branch, and per side of each gate, of the two dispatchers that carry
almost all of the project's FLOPs -- kd_conv2d_fwd (csrc/conv_igemm.hip) and kd_conv2d_wgrad / kd_pw_wgrad (csrc/pw_wgrad.hip), whose
selections are conv_select / wgrad_select of csrc/conv_select.h -- together with a pure-Python restatement of both selections for
the default environment (no KDCC_* switch set).  tests/test_conv_dispatch_host.py evaluates the restatement on every row without a
GPU and tests/test_conv_select_host.py holds it against the C selection; on the GPU the same name is compared with the dispatcher's
own log.  Nothing here imports torch or touches the device.

Every limit is read off the source:
  conv_igemm.hip  CfgRowT::MAXDIL = (AROWS - BM) / 2: CfgRow (320 rows) 32, CfgRowX (384) 64, CfgRowN (384) 64;
  conv_select.h   conv_select: cfg = wide iff Cout > 128 and ceil(M / 256) * ceil(Cout / 256) >= 224; row geometry = 3x3, stride 1,
                  pad == dil, W % 256 == 0; persist_ok = bf16, wide, vec_ok, !raw_f32, M % 256 == 0, Cout % 256 == 0;
                  use_pp128 = narrow row geometry, vec_ok, !raw_f32, <= 2 operands, Cout % 128 == 0, W % 512 == 0, dil <= 16;
                  conv_row_lw_kernel iff H >= 2 dil, conv_row_tall_kernel iff Cin % 64 == 0 and H > dil;
                  tn_group = 4 iff Cout / 256 > 4 and (Cout / 256) % 4 == 0;
                  WR_XROWS = 96 (row_eligible: 2 dil + 64 <= 96, i.e. dil <= 16), conv_wgrad_lw_kernel iff Cout % 128 == 0 and
                  dil <= 8, wide_tile_pays (>= 256 channels on both sides, padding of 256-tiles <= 135 % of 128-tiles),
                  pw_lw_pays (Cin % 256, Cout % 256, M % 64, rps % 32), plan / wide_plan / row_plan / fill_splits.

What the source makes unreachable at default settings (so there is no row for it; the host test pins the reasoning):
  * kd_conv2d_fwd refuses Cin % (128 / elem size) != 0 before it selects, so a bf16 Cin of 32 or 96 never reaches the 512 x 128
    tiles: `Cin % 32` of use_pp128 and `Cin % 64` of the conv_row_tall_kernel gate are always true (REFUSED_CIN is checked on the GPU);
  * output sums without operands are only granted on the 1x1 ping-pong kernel (kd_conv2d_bn_sums_rows, no-mask arm), so the
    `bn_sums && nops == 0` term of the conv_row_tall_kernel gate is never false on the 512 x 128 tiles: conv_row_pp128_kernel is
    reached by H <= dil alone;
  * wide_plan's rps is (stages per split) * 64, so `rps % 32` of pw_lw_pays never fails; M % 64 is its only live pixel gate;
  * the 135 % rule: the source's comment names the decoder's 304 -> 256 layer, which is INSIDE (2 x 256 against 3 x 128 columns is
    133 %); the first outside neighbour has both sides ragged (304 x 304: 4 tiles of 256 against 9 of 128, 178 %).
"""
import zlib

CASES = []

# names the source declares that no default-environment problem reaches: name -> the switch that does.  Proofs, from conv_select /
# conv2d_fwd_impl: c.half, cfg 2 and cfg 3 are only ever set inside the KDCC_CONV_CFG block; duo_ok needs duo > 0 (KDCC_CONV_DUO);
# <dbg> needs tune & 512 (KDCC_CONV_TUNE, tuning build); both <lockstep> arms need !pp_row() -- the row one could also be reached by
# dil > 32, but use_row_persist excludes row_x (dil > CfgRow::MAXDIL = 32) -- and conv_pw_lw_kernel needs lw_pw (opt-in).
SWITCH_ONLY = {
    "conv_igemm_kernel<half>": "KDCC_CONV_CFG=half",
    "conv_igemm_row_kernel<half>": "KDCC_CONV_CFG=half",
    "conv_igemm_kernel<deep>": "KDCC_CONV_CFG=deep",
    "conv_igemm_kernel<f32,deep>": "KDCC_CONV_CFG=deep",
    "conv_igemm_kernel<narrow>": "KDCC_CONV_CFG=narrow1",
    "conv_row_persist_kernel<lockstep>": "KDCC_CONV_PP=0",
    "conv_igemm_persist_kernel<lockstep>": "KDCC_CONV_PP=0",
    "conv_row_persist_kernel<dbg>": "KDCC_CONV_TUNE=512",
    "conv_row_duo_kernel": "KDCC_CONV_DUO=1",
    "conv_pw_lw_kernel": "KDCC_CONV_LW_PW=1",
}

# literals the forward dispatcher notes NEXT TO the kernel that carries them (they count epilogues, not kernels)
EPILOGUE_NOTES = ("bn_sums_epilogue", "out_sums_epilogue", "cls_epilogue")

# bf16 reduction depths kd_conv2d_fwd refuses before selecting (Cin % 64), on the shape that would otherwise test `Cin % 64` of the
# conv_row_tall_kernel gate
REFUSED_CIN = (32, 96)

ROW_MAXDIL, ROWX_MAXDIL, ROWN_MAXDIL = (320 - 256) // 2, (384 - 256) // 2, (384 - 256) // 2
WIDE_TILES_MIN = 224
WR_XROWS = 96
WGRAD_ROW_MAXDIL = (WR_XROWS - 64) // 2
WS_SPLIT_CAP = 768

# every gate the table must sit on, with the sides it must show
GATES = {
    "fwd.wide_tiles>=224": ("below", "at"),
    "fwd.Cout>128": ("128", "136", "256"),
    "fwd.row_geom.pad==dil": ("on", "off"),
    "fwd.row_geom.W%256": ("on", "off"),
    "fwd.row_geom.stride": ("on", "off"),
    "fwd.row_geom.3x3": ("on", "off"),
    "fwd.narrow_row_geom.W%256": ("on", "off"),
    "fwd.CfgRow.MAXDIL": ("at", "past"),
    "fwd.CfgRowX.MAXDIL": ("at", "past"),
    "fwd.CfgRowN.MAXDIL": ("at", "past"),
    "fwd.f32.CfgRow.MAXDIL": ("at", "past"),
    "fwd.f32.CfgRowX.MAXDIL": ("at", "past"),
    "fwd.f32.narrow_row": ("never",),
    "fwd.row_persist.H>=2dil": ("H=dil", "H=2dil-1", "H=2dil"),
    "fwd.pp128.H>dil": ("H=dil", "H=dil+1"),
    "fwd.persist.Cout%256": ("on", "off"),
    "fwd.persist.raw_f32": ("on", "off"),
    "fwd.persist.vec_ok": ("on", "operand", "output"),
    "fwd.persist.nops<=3": ("2", "3"),
    "fwd.igemm_persist.Cout%256": ("on", "off"),
    "fwd.igemm_persist.raw_f32": ("on", "off"),
    "fwd.igemm_persist.vec_ok": ("on", "off"),
    "fwd.pp128.W%512": ("256", "512"),
    "fwd.pp128.dil<=16": ("16", "17"),
    "fwd.pp128.Cin": ("64", "128"),
    "fwd.pp128.nops<=2": ("2", "3"),
    "fwd.pp128.Cout%128": ("128", "136", "256"),
    "fwd.pp128.raw_f32": ("on", "off"),
    "fwd.pp128.sums": ("mask", "mask,H=dil", "none"),
    "fwd.tn_group.1x1": ("4", "5", "8"),
    "fwd.tn_group.row": ("4", "5", "8"),
    "fwd.grid.row": ("fewer", "ragged0", "ragged1", "ragged2"),
    "fwd.grid.1x1": ("fewer", "ragged0", "ragged1", "ragged2"),
    "fwd.grid.pp128": ("fewer", "ragged"),
    "fwd.dual": ("on",),
    "fwd.cls": ("on",),
    "fwd.out_sums": ("on",),
    "fwd.bn_sums.row": ("on",),
    "fwd.dgrad": ("row", "1x1", "narrow"),
    "wgrad.row.Cout%128": ("128", "136"),
    "wgrad.row.dil<=8": ("8", "9"),
    "wgrad.row.WR_XROWS": ("at", "past,small", "past,wide"),
    "wgrad.row.W%64": ("64", "72"),
    "wgrad.row.bf16": ("f32",),
    "wgrad.wide.Cin>=256": ("248", "256"),
    "wgrad.wide.Cout>=256": ("248", "256"),
    "wgrad.wide.135%": ("inside", "outside"),
    "wgrad.wide.Cin%8": ("off",),
    "wgrad.wide.geom": ("1x1", "3x3"),
    "wgrad.pw_lw.M%64": ("on", "off"),
    "wgrad.generic": ("tr", "bf16", "f32"),
    "wgrad.plan.stages": ("one", "under4", "one,row", "under8,row"),
    "wgrad.plan.cap768": ("tr", "wide"),
    "wgrad.reduce.n%4": ("on", "off"),
    "pw.wide.Cin>=256": ("248", "256"),
    "pw.wide.135%": ("inside", "outside"),
    "pw.generic": ("tr", "bf16", "f32"),
    "pw.pw_lw.M%64": ("on", "off"),
}


def fwd(cid, dt, shape, kernel, gates, reason, ops=(), outs=("raw",), **kw):
    """shape = (N, H, W, Cin, Cout, k, stride, pad, dil) of the convolution kd_conv2d_fwd is handed."""
    CASES.append(dict(id=f"fwd:{cid}", entry="conv2d", dt=dt, shape=shape, ops=tuple(ops), outs=tuple(outs), kernel=kernel,
                      gates=tuple(gates), reason=reason, **kw))


def dgrad(cid, dt, shape, kernel, gates, reason, ops=(), outs=("raw",), **kw):
    """shape = the FORWARD layer; the dispatcher sees its input gradient: a stride-1 'same' conv Cout -> Cin with a KD_PACK_DGRAD weight."""
    CASES.append(dict(id=f"dgrad:{cid}", entry="conv2d_dgrad", dt=dt, shape=shape, ops=tuple(ops), outs=tuple(outs), kernel=kernel,
                      gates=tuple(gates), reason=reason, **kw))


def wgrad(cid, dt, shape, kernel, gates, reason, **kw):
    CASES.append(dict(id=f"wgrad:{cid}", entry="conv2d_wgrad", dt=dt, shape=shape, kernel=kernel, gates=tuple(gates), reason=reason, **kw))


def pw(cid, dt, shape, kernel, gates, reason, **kw):
    """shape = (N, H, W, Cin, Cout)."""
    CASES.append(dict(id=f"pw:{cid}", entry="pw_wgrad", dt=dt, shape=tuple(shape) + (1, 1, 0, 1), kernel=kernel, gates=tuple(gates),
                      reason=reason, **kw))


def ids(cs):
    return [c["id"] for c in cs]


def cases_of(*entries):
    return [c for c in CASES if c["entry"] in entries]


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


# ====================================================================================================== restated selection
def conv_out(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


def seen_shape(c):
    """The problem the dispatcher is handed: (N, H, W, Cin, Cout, k, stride, pad, dil)."""
    N, H, W, Cin, Cout, k, s, p, d = c["shape"]
    if c["entry"] == "conv2d_dgrad":
        assert s == 1 and p == d * (k // 2)
        return (N, H, W, Cout, Cin, k, 1, p, d)
    if c["entry"] == "conv2d" and c.get("cin2"):
        return (N, H, W, Cin + c["cin2"], Cout, k, s, p, d)
    return c["shape"]


def fwd_select(c, ncu=256):
    """conv_select + the branch order of conv2d_fwd_impl, default environment -> dict(kernel, notes, grid, ntiles, tn_group)."""
    N, H, W, Cin, Cout, k, s, p, d = seen_shape(c)
    bf16 = c["dt"] == "bf16"
    Ho, Wo = conv_out(H, k, s, p, d), conv_out(W, k, s, p, d)
    M = N * Ho * Wo
    raw_f32 = bool(c.get("raw_f32")) and bf16
    vec_ok = not c.get("misalign")
    nops = len(c["ops"])
    sums = c.get("sums")                     # "bn" (with mask) | "out" (no operand) | None
    wide_tiles = -(-M // 256) * -(-Cout // 256)
    cfg = 1 if (Cout > 128 and wide_tiles >= WIDE_TILES_MIN) else 0
    row_geom = k == 3 and s == 1 and p == d and W % 256 == 0
    row_wide = row_geom and cfg == 1 and d <= ROWX_MAXDIL
    row_x = row_wide and d > ROW_MAXDIL
    row_narrow = row_geom and cfg == 0 and bf16 and d <= ROWN_MAXDIL
    persist_ok = bf16 and cfg == 1 and vec_ok and not raw_f32 and M % 256 == 0 and Cout % 256 == 0   # (nops <= 2 or ping-pong: default)
    use_row_persist = persist_ok and row_wide and not row_x
    use_igemm_persist = not use_row_persist and persist_ok and k == 1 and s == 1 and p == 0
    use_pp128 = (not use_row_persist and not use_igemm_persist and row_narrow and vec_ok and not raw_f32 and nops <= 2 and
                 Cout % 128 == 0 and W % 512 == 0 and d <= 16 and Cin % 32 == 0)
    # kd_conv2d_bn_sums_rows: which kernels take the sums
    if sums == "out":
        granted = use_igemm_persist and nops == 0 and "raw" in c["outs"] and "act" not in c["outs"] and not raw_f32
    elif sums == "bn":
        granted = (use_row_persist or use_igemm_persist or use_pp128) and nops <= 2 and "mask" in c["ops"]
    else:
        granted = False
    notes = []
    if granted:
        notes.append("bn_sums_epilogue" if "mask" in c["ops"] else "out_sums_epilogue")
    if c.get("cls"):
        assert use_row_persist and nops == 0 and Cout == 256 and H >= 2 * d, "the classifier epilogue needs conv_row_lw_kernel"
        notes.append("cls_epilogue")
    pcus = ncu - ncu % 8
    out = dict(notes=tuple(notes), sums_granted=granted, tn_group=None, ntiles=None, grid=None)

    def persist_grid(ntiles):
        out["ntiles"] = ntiles
        out["grid"] = (min(ntiles, pcus) + 7) // 8 * 8

    if c.get("cin2"):
        assert use_igemm_persist, "the K-concatenated 1x1 conv needs conv_igemm_persist_kernel<pp>"
    if use_row_persist or use_igemm_persist:
        tn = Cout // 256
        out["tn_group"] = 4 if (tn > 4 and tn % 4 == 0) else 0
        persist_grid((M // 256) * tn)
        if use_row_persist:
            out["kernel"] = "conv_row_lw_kernel" if H >= 2 * d else "conv_row_persist_kernel<pp>"
        else:
            out["kernel"] = "conv_igemm_persist_kernel<pp,dual>" if c.get("cin2") else "conv_igemm_persist_kernel<pp>"
    elif use_pp128:
        persist_grid((M // 512) * (Cout // 128))
        tall = Cin % 64 == 0 and H > d and not (granted and nops == 0)
        out["kernel"] = "conv_row_tall_kernel" if tall else "conv_row_pp128_kernel"
    elif row_wide or row_narrow:
        if row_narrow:
            out["kernel"] = "conv_igemm_row_kernel<narrow>"
        elif row_x:
            out["kernel"] = "conv_igemm_row_kernel<x>" if bf16 else "conv_igemm_row_kernel<f32,x>"
        else:
            out["kernel"] = "conv_igemm_row_kernel<wide>" if bf16 else "conv_igemm_row_kernel<f32,wide>"
    elif bf16:
        out["kernel"] = "conv_igemm_kernel<wide>" if cfg == 1 else "conv_igemm_kernel<narrow2>"
    else:
        out["kernel"] = "conv_igemm_kernel<f32,wide>" if cfg == 1 else "conv_igemm_kernel<f32,narrow>"
    return out


def plan(dt, M, Cin, Cout, taps=1):
    krows = 128 // (2 if dt == "bf16" else 4)
    tiles = -(-Cin // 128) * -(-Cout // 128)
    stages = -(-M // krows)
    want = -(-1024 // (tiles * taps))
    max_splits = (stages + 3) // 4
    splits = max(1, min(want, max_splits))
    rps = -(-stages // splits) * krows
    return dict(tiles=tiles, splits=-(-M // rps), rps=rps, stages=stages)


def fill_splits(per, max_splits):
    splits, best = 1, -1.0
    for k in range(1, 5):
        sp = max(1, min((256 * k) // per, max_splits))
        w = sp * per
        fill = w / (-(-w // 256) * 256)
        if fill >= 0.95:
            return sp
        if fill > best:
            best, splits = fill, sp
    return splits


def wide_plan(M, Cin, Cout, taps):
    tiles = -(-Cin // 256) * -(-Cout // 256)
    stages = -(-M // 64)
    max_splits = (stages + 7) // 8
    splits = max(1, min(fill_splits(tiles * taps, max_splits), max_splits))
    rps = -(-stages // splits) * 64
    return dict(tiles=tiles, splits=-(-M // rps), rps=rps, stages=stages)


def row_plan(M, Cin, Cout):
    tiles = -(-Cin // 128) * -(-Cout // 128)
    stages = M // 64
    max_splits = (stages + 7) // 8
    splits = max(1, min(fill_splits(tiles * 3, max_splits), max_splits))
    rps = -(-stages // splits) * 64
    return dict(tiles=tiles, splits=-(-M // rps), rps=rps, stages=stages)


def wide_tile_pays(dt, Cin, Cout):
    pad256 = -(-Cout // 256) * -(-Cin // 256) * 65536
    pad128 = -(-Cout // 128) * -(-Cin // 128) * 16384
    return dt == "bf16" and Cin % 8 == 0 and Cout % 8 == 0 and Cout >= 256 and Cin >= 256 and pad256 * 100 <= pad128 * 135


def row_eligible(dt, Cin, Cout, W, k, s, p, d):
    return dt == "bf16" and k == 3 and s == 1 and p == d and 2 * d + 64 <= WR_XROWS and W % 64 == 0 and Cin % 8 == 0 and Cout % 8 == 0


def wgrad_select(c):
    """kd_conv2d_wgrad / kd_pw_wgrad, default environment -> dict(kernel, splits, rps, need, workspace, reduce4)."""
    N, H, W, Cin, Cout, k, s, p, d = c["shape"]
    dt = c["dt"]
    M = N * conv_out(H, k, s, p, d) * conv_out(W, k, s, p, d)
    taps = k * k
    pl = plan(dt, M, Cin, Cout, taps)
    wide = wide_tile_pays(dt, Cin, Cout)
    row = c["entry"] == "conv2d_wgrad" and row_eligible(dt, Cin, Cout, W, k, s, p, d)
    if row:
        pl = row_plan(M, Cin, Cout)
        kernel = "conv_wgrad_lw_kernel" if (Cout % 128 == 0 and d <= 8) else "conv_wgrad_row_kernel"
    elif wide:
        pl = wide_plan(M, Cin, Cout, taps)
        geom = not (taps == 1 and s == 1 and p == 0)
        lw = not geom and Cin % 256 == 0 and Cout % 256 == 0 and M % 64 == 0 and pl["rps"] % 32 == 0
        kernel = "conv_wgrad_pw_lw_kernel" if lw else "conv_wgrad_wide_kernel"
    elif dt == "bf16" and Cin % 8 == 0 and Cout % 8 == 0:
        kernel = "pw_wgrad_tr_kernel"
    else:
        kernel = "pw_wgrad_kernel<bf16>" if dt == "bf16" else "pw_wgrad_kernel<f32>"
    # the ABI's workspace bound (kd_conv2d_wgrad_workspace / kd_pw_wgrad_workspace)
    stages = -(-M // 64)
    bound = max(plan("f32", M, Cin, Cout, taps)["splits"], plan("bf16", M, Cin, Cout, taps)["splits"], min((stages + 7) // 8, WS_SPLIT_CAP))
    if row:
        bound = max(bound, row_plan(M, Cin, Cout)["splits"])
    n = Cout * Cin * taps
    return dict(kernel=kernel, splits=pl["splits"], rps=pl["rps"], stages=pl["stages"], need=pl["splits"] * n * 4, workspace=bound * n * 4,
                reduce4=(taps == 1 and n % 4 == 0), notes=())


def predict(c, ncu=256):
    return fwd_select(c, ncu) if c["entry"] in ("conv2d", "conv2d_dgrad") else wgrad_select(c)


# ============================================================================================================ forward table
L, LW, P, X = "conv_row_lw_kernel", "conv_igemm_row_kernel<wide>", "conv_igemm_persist_kernel<pp>", "conv_igemm_row_kernel<x>"
G, G2, NR = "conv_igemm_kernel<wide>", "conv_igemm_kernel<narrow2>", "conv_igemm_row_kernel<narrow>"
FW, FX, FG, FN = "conv_igemm_row_kernel<f32,wide>", "conv_igemm_row_kernel<f32,x>", "conv_igemm_kernel<f32,wide>", "conv_igemm_kernel<f32,narrow>"
TALL, PP128, RPP = "conv_row_tall_kernel", "conv_row_pp128_kernel", "conv_row_persist_kernel<pp>"

# ---- the tile-count threshold and Cout > 128 (1x1 layers: the reduction is one K stage, the oracle stays cheap)
fwd("thr.1x1.223", "bf16", (1, 223, 256, 64, 256, 1, 1, 0, 1), G2, [("fwd.wide_tiles>=224", "below")],
    "223 wide tiles: one under the threshold, the 256 x 128 gather kernel takes a 256-channel 1x1 (two N tiles)")
fwd("thr.1x1.224", "bf16", (1, 224, 256, 64, 256, 1, 1, 0, 1), P,
    [("fwd.wide_tiles>=224", "at"), ("fwd.Cout>128", "256"), ("fwd.igemm_persist.Cout%256", "on"), ("fwd.igemm_persist.raw_f32", "off"),
     ("fwd.igemm_persist.vec_ok", "on"), ("fwd.grid.1x1", "fewer"), ("fwd.row_geom.3x3", "off")],
    "224 wide tiles: the first wide shape; a persistent grid of 224 workgroups, fewer tiles than a 256-CU chip has workgroups")
fwd("thr.3x3.223", "bf16", (1, 223, 256, 64, 256, 3, 1, 1, 1), NR, [("fwd.wide_tiles>=224", "below"), ("fwd.pp128.W%512", "256"), ("fwd.pp128.Cout%128", "256")],
    "223 wide tiles, row geometry: the narrow row kernel with two N tiles of 128 (W = 256 keeps it off the 512 x 128 tiles)")
fwd("thr.3x3.224", "bf16", (1, 224, 256, 64, 256, 3, 1, 1, 1), L,
    [("fwd.wide_tiles>=224", "at"), ("fwd.row_geom.pad==dil", "on"), ("fwd.row_geom.W%256", "on"), ("fwd.row_geom.stride", "on"), ("fwd.row_geom.3x3", "on"),
     ("fwd.persist.Cout%256", "on"), ("fwd.persist.raw_f32", "off"), ("fwd.persist.vec_ok", "on"), ("fwd.grid.row", "fewer")],
    "224 wide tiles, row geometry: the base layer of the persistent row path (every later `leaves by one reason` row edits this one)",
    wkey_cout=320)
fwd("thr.f32.1x1.223", "f32", (1, 223, 256, 32, 256, 1, 1, 0, 1), FN, [("fwd.wide_tiles>=224", "below")],
    "fp32, 223 wide tiles: the fp32 narrow gather kernel")
fwd("thr.f32.1x1.224", "f32", (1, 224, 256, 32, 256, 1, 1, 0, 1), FG, [("fwd.wide_tiles>=224", "at")],
    "fp32, 224 wide tiles: the fp32 wide gather kernel (fp32 has no persistent kernel)")
fwd("cout.128", "bf16", (1, 224, 256, 64, 128, 1, 1, 0, 1), G2, [("fwd.Cout>128", "128")],
    "Cout = 128 at 224 M tiles: `Cout > 128` false, narrow tiles however many there are")
fwd("cout.136", "bf16", (1, 224, 256, 64, 136, 1, 1, 0, 1), G, [("fwd.Cout>128", "136"), ("fwd.igemm_persist.Cout%256", "off")],
    "Cout = 136: wide tiles with a ragged N tile of 136 channels, Cout % 256 != 0 keeps it off the persistent 1x1 kernel")
fwd("cout.f32.128", "f32", (1, 224, 256, 32, 128, 1, 1, 0, 1), FN, [("fwd.Cout>128", "128")], "fp32, Cout = 128: narrow")
fwd("cout.f32.136", "f32", (1, 224, 256, 32, 136, 1, 1, 0, 1), FG, [("fwd.Cout>128", "136")], "fp32, Cout = 136: wide tiles, ragged N tile")

# ---- row geometry off by one predicate at a time (from thr.3x3.224)
fwd("geom.pad", "bf16", (1, 228, 256, 64, 256, 3, 1, 1, 2), G, [("fwd.row_geom.pad==dil", "off")],
    "pad 1, dil 2: the output is 226 x 254, rows are not tile segments -> gathered im2col on wide tiles (225 of them, ragged last M tile)")
fwd("geom.w264", "bf16", (1, 218, 264, 64, 256, 3, 1, 1, 1), G, [("fwd.row_geom.W%256", "off")],
    "W = 264: W % 256 != 0 -> gathered im2col (225 wide tiles)")
fwd("geom.stride2", "bf16", (1, 448, 512, 64, 256, 3, 2, 1, 1), G, [("fwd.row_geom.stride", "off")],
    "stride 2 onto 224 x 256 outputs: whole tiles and Cout % 256 == 0, but neither row geometry nor 1x1 -> gathered im2col")
fwd("geom.narrow.w256", "bf16", (1, 4, 256, 64, 128, 3, 1, 1, 1), NR, [("fwd.narrow_row_geom.W%256", "on")],
    "narrow tiles, row geometry, W = 256: the narrow row kernel, every output row at an image border for some kernel row")
fwd("geom.narrow.w264", "bf16", (1, 4, 264, 64, 128, 3, 1, 1, 1), G2, [("fwd.narrow_row_geom.W%256", "off")],
    "narrow tiles, W = 264: gathered im2col on 256 x 128 tiles, ragged last M tile")
fwd("geom.f32.narrow", "f32", (1, 4, 256, 32, 128, 3, 1, 1, 1), FN, [("fwd.f32.narrow_row", "never")],
    "fp32 with narrow row geometry: row_narrow needs bf16, fp32 takes the gather kernel")

# ---- dilation at and one past each row buffer's MAXDIL, H >= 2 dil: kernel rows leave the image at the top and at the bottom
fwd("dil.row.32", "bf16", (1, 224, 256, 64, 256, 3, 1, 32, 32), L, [("fwd.CfgRow.MAXDIL", "at")],
    "dil = CfgRow::MAXDIL = 32: the last dilation of the 320-row buffer (256 + 2 * 32 rows staged), lone-wave kernel")
fwd("dil.row.33", "bf16", (1, 224, 256, 64, 256, 3, 1, 33, 33), X, [("fwd.CfgRow.MAXDIL", "past")],
    "dil = 33: row_x, the 384-row buffer; use_row_persist excludes it")
fwd("dil.rowx.64", "bf16", (1, 224, 256, 64, 256, 3, 1, 64, 64), X, [("fwd.CfgRowX.MAXDIL", "at")],
    "dil = CfgRowX::MAXDIL = 64: all 384 rows of the buffer in use")
fwd("dil.rowx.65", "bf16", (1, 224, 256, 64, 256, 3, 1, 65, 65), G, [("fwd.CfgRowX.MAXDIL", "past")],
    "dil = 65: past every row buffer, falls to the gather kernel")
fwd("dil.f32.32", "f32", (1, 224, 256, 32, 256, 3, 1, 32, 32), FW, [("fwd.f32.CfgRow.MAXDIL", "at")], "fp32, dil = 32: CfgRowF")
fwd("dil.f32.33", "f32", (1, 224, 256, 32, 256, 3, 1, 33, 33), FX, [("fwd.f32.CfgRow.MAXDIL", "past")], "fp32, dil = 33: CfgRowXF")
fwd("dil.f32.64", "f32", (1, 224, 256, 32, 256, 3, 1, 64, 64), FX, [("fwd.f32.CfgRowX.MAXDIL", "at")], "fp32, dil = 64: last dilation of CfgRowXF")
fwd("dil.f32.65", "f32", (1, 224, 256, 32, 256, 3, 1, 65, 65), FG, [("fwd.f32.CfgRowX.MAXDIL", "past")], "fp32, dil = 65: the fp32 wide gather kernel")
fwd("dil.rown.64", "bf16", (1, 128, 256, 64, 128, 3, 1, 64, 64), NR, [("fwd.CfgRowN.MAXDIL", "at")],
    "narrow row kernel at CfgRowN::MAXDIL = 64, H = 2 dil: every output row has exactly two kernel rows inside the image")
fwd("dil.rown.65", "bf16", (1, 130, 256, 64, 128, 3, 1, 65, 65), G2, [("fwd.CfgRowN.MAXDIL", "past")],
    "narrow tiles, dil = 65: gathered im2col")

# ---- H against dil on the persistent row path (dil 8: 224 tiles need N * H >= 224) and on the 512 x 128 tiles
fwd("h.row.dil", "bf16", (28, 8, 256, 64, 256, 3, 1, 8, 8), RPP, [("fwd.row_persist.H>=2dil", "H=dil")],
    "H = dil: only the centre kernel row is ever inside the image -> the ping-pong kernel, which counts kernel rows per tile", ops=("pre",), outs=("raw", "act"))
fwd("h.row.2dil-1", "bf16", (15, 15, 256, 64, 256, 3, 1, 8, 8), RPP, [("fwd.row_persist.H>=2dil", "H=2dil-1")],
    "H = 2 dil - 1: output row dil - 1 has ONE kernel row inside the image, the lone-wave loop's hand-over assumes two -> ping-pong kernel",
    ops=("mask",), outs=("raw", "act"))
fwd("h.row.2dil", "bf16", (15, 16, 256, 64, 256, 3, 1, 8, 8), L, [("fwd.row_persist.H>=2dil", "H=2dil")],
    "H = 2 dil: the first height of the lone-wave kernel; the data of h.row.2dil-1 with one zero row appended, so rows 0..14 must agree",
    ops=("mask",), outs=("raw", "act"), zero_rows=1, pair=("fwd:h.row.2dil-1", "rows"))
fwd("h.tall.dil", "bf16", (2, 4, 512, 64, 128, 3, 1, 4, 4), PP128, [("fwd.pp128.H>dil", "H=dil"), ("fwd.grid.pp128", "fewer")],
    "512 x 128 tiles, H = dil: no output row has a second kernel row -> conv_row_pp128_kernel (8 tiles, one grid round of 8)", ops=("pre",), outs=("raw", "act"))
fwd("h.tall.dil+1", "bf16", (2, 5, 512, 64, 128, 3, 1, 4, 4), TALL, [("fwd.pp128.H>dil", "H=dil+1")],
    "512 x 128 tiles, H = dil + 1: first height of conv_row_tall_kernel; h.tall.dil's data plus one zero row", ops=("pre",), outs=("raw", "act"),
    zero_rows=1, pair=("fwd:h.tall.dil", "rows"))

# ---- leaving the persistent kernels one reason at a time
fwd("leave.cout320", "bf16", (1, 224, 256, 64, 320, 3, 1, 1, 1), LW, [("fwd.persist.Cout%256", "off")],
    "Cout = 320: a ragged second N tile -> bf16 conv_igemm_row_kernel<wide>; its first 256 channels are thr.3x3.224's layer",
    pair=("fwd:thr.3x3.224", "channels"))
fwd("leave.raw_f32", "bf16", (1, 224, 256, 64, 256, 3, 1, 1, 1), LW, [("fwd.persist.raw_f32", "on")],
    "an fp32 raw output next to the bf16 activation: the fp32 epilogue patch, one tile per workgroup", ops=("pre",), outs=("raw", "act"), raw_f32=True)
fwd("leave.misaligned_operand", "bf16", (1, 224, 256, 64, 256, 3, 1, 1, 1), LW, [("fwd.persist.vec_ok", "operand")],
    "res_pre is a view 8 bytes into its buffer: vec_ok false, the guarded scalar epilogue of the one-tile row kernel", ops=("pre", "mask"),
    outs=("raw", "act"), misalign="pre")
fwd("leave.misaligned_output", "bf16", (1, 224, 256, 64, 256, 3, 1, 1, 1), LW, [("fwd.persist.vec_ok", "output")],
    "out_raw is a view 8 bytes into its buffer: vec_ok false through an output", ops=("post",), outs=("raw", "act"), misalign="raw")
fwd("stay.three_operands", "bf16", (1, 224, 256, 64, 256, 3, 1, 1, 1), L, [("fwd.persist.nops<=3", "3")],
    "three operands: the default (ping-pong / lone-wave) instantiations take them, the launch stays persistent", ops=("pre", "mask", "post"),
    outs=("raw", "act"))
fwd("stay.two_operands", "bf16", (1, 224, 256, 64, 256, 3, 1, 1, 1), L, [("fwd.persist.nops<=3", "2"), ("fwd.bn_sums.row", "on")],
    "two operands and the eval-BN parameter sums in the epilogue of the lone-wave kernel", ops=("pre", "mask"), outs=("raw",), sums="bn")
fwd("leave.1x1.raw_f32", "bf16", (1, 224, 256, 64, 256, 1, 1, 0, 1), G, [("fwd.igemm_persist.raw_f32", "on")],
    "1x1 with an fp32 raw output: the one-tile wide gather kernel", raw_f32=True)
fwd("leave.1x1.misaligned", "bf16", (1, 224, 256, 64, 256, 1, 1, 0, 1), G, [("fwd.igemm_persist.vec_ok", "off")],
    "1x1 whose mask is a view 8 bytes into its buffer", ops=("mask",), outs=("raw", "act"), misalign="mask")

# ---- the 512 x 128 tiles
fwd("pp128.w512", "bf16", (1, 8, 512, 64, 128, 3, 1, 1, 1), TALL, [("fwd.pp128.W%512", "512"), ("fwd.pp128.Cin", "64"), ("fwd.pp128.Cout%128", "128"), ("fwd.pp128.raw_f32", "off")],
    "W = 512, Cout = 128, Cin = one 64-channel pair of K stages: the smallest conv_row_tall_kernel launch (8 tiles)")
fwd("pp128.w256", "bf16", (1, 16, 256, 64, 128, 3, 1, 1, 1), NR, [("fwd.pp128.W%512", "256")], "W = 256: no 512-pixel tiles, the narrow row kernel")
fwd("pp128.dil16", "bf16", (1, 34, 512, 64, 128, 3, 1, 16, 16), TALL, [("fwd.pp128.dil<=16", "16")], "dil = 16, the last dilation of the 512 x 128 tiles, H >= 2 dil",
    ops=("mask", "post"), outs=("raw", "act"))
fwd("pp128.dil17", "bf16", (1, 34, 512, 64, 128, 3, 1, 17, 17), NR, [("fwd.pp128.dil<=16", "17")], "dil = 17: back to the narrow row kernel",
    ops=("mask", "post"), outs=("raw", "act"))
fwd("pp128.cin128", "bf16", (1, 8, 512, 128, 128, 3, 1, 2, 2), TALL, [("fwd.pp128.Cin", "128")],
    "Cin = 128: two pairs of K stages (Cin = 32 / 96 are refused by kd_conv2d_fwd before it selects: REFUSED_CIN)", ops=("pre", "post"), outs=("act",))
fwd("pp128.two_operands", "bf16", (1, 8, 512, 64, 128, 3, 1, 1, 1), TALL, [("fwd.pp128.nops<=2", "2")], "two operands stay on the 512 x 128 tiles",
    ops=("pre", "mask"), outs=("raw", "act"))
fwd("pp128.three_operands", "bf16", (1, 8, 512, 64, 128, 3, 1, 1, 1), NR, [("fwd.pp128.nops<=2", "3")], "three operands: no 512 x 128 instantiation, the narrow row kernel",
    ops=("pre", "mask", "post"), outs=("raw", "act"))
fwd("pp128.cout136", "bf16", (1, 8, 512, 64, 136, 3, 1, 1, 1), NR, [("fwd.pp128.Cout%128", "136")],
    "Cout = 136 under 224 wide tiles: narrow tiles with a ragged second N tile of 8 channels")
fwd("pp128.cout256", "bf16", (1, 8, 512, 64, 256, 3, 1, 1, 1), TALL, [("fwd.pp128.Cout%128", "256")],
    "Cout = 256 under 224 wide tiles: narrow config, TWO N tiles of 128 on the 512 x 128 kernel (16 tiles)", ops=("pre",), outs=("raw", "act"))
fwd("pp128.raw_f32", "bf16", (1, 8, 512, 64, 128, 3, 1, 1, 1), NR, [("fwd.pp128.raw_f32", "on")], "an fp32 raw output leaves the 512 x 128 tiles", raw_f32=True)
fwd("pp128.sums.mask", "bf16", (1, 8, 512, 64, 128, 3, 1, 1, 1), TALL, [("fwd.pp128.sums", "mask")], "eval-BN sums with mask + res_post on conv_row_tall_kernel",
    ops=("mask", "post"), outs=("raw",), sums="bn")
fwd("pp128.sums.mask.h=dil", "bf16", (2, 4, 512, 64, 128, 3, 1, 4, 4), PP128, [("fwd.pp128.sums", "mask,H=dil")],
    "eval-BN sums on conv_row_pp128_kernel (H = dil): its <5> instantiation, which no other default-environment test launches", ops=("mask",), outs=("raw",), sums="bn")
fwd("pp128.sums.none", "bf16", (1, 8, 512, 64, 128, 3, 1, 1, 1), TALL, [("fwd.pp128.sums", "none")],
    "output sums asked without operands: kd_conv2d_bn_sums_rows grants them on the 1x1 ping-pong kernel only, so none are produced and the kernel stays",
    sums="out")
fwd("pp128.grid.ragged", "bf16", (1, 136, 1024, 64, 128, 3, 1, 1, 1), TALL, [("fwd.grid.pp128", "ragged")],
    "272 tiles of 512 pixels: more than any CU count up to 264, some workgroups walk a second tile", ops=("pre",), outs=("raw", "act"))

# ---- N-tile grouping of the persistent grid (tn_group): 4, 5 and 8 tiles of 256 channels
fwd("tn.1x1.1024", "bf16", (1, 28, 512, 64, 1024, 1, 1, 0, 1), P, [("fwd.tn_group.1x1", "4")], "four N tiles: tiles_n > 4 false, plain walk", tn_group=0)
fwd("tn.1x1.1280", "bf16", (1, 45, 256, 64, 1280, 1, 1, 0, 1), P, [("fwd.tn_group.1x1", "5")], "five N tiles: tiles_n % 4 != 0, plain walk (225 tiles)", tn_group=0,
    ops=("pre",), outs=("raw", "act"))
fwd("tn.1x1.2048", "bf16", (1, 14, 512, 64, 2048, 1, 1, 0, 1), P, [("fwd.tn_group.1x1", "8")], "eight N tiles: walked four at a time over all M tiles", tn_group=4,
    ops=("mask",), outs=("raw", "act"))
fwd("tn.row.1024", "bf16", (1, 56, 256, 64, 1024, 3, 1, 1, 1), L, [("fwd.tn_group.row", "4")], "row kernel, four N tiles: plain walk", tn_group=0)
fwd("tn.row.1280", "bf16", (1, 45, 256, 64, 1280, 3, 1, 2, 2), L, [("fwd.tn_group.row", "5")], "row kernel, five N tiles: plain walk (225 tiles)", tn_group=0,
    ops=("post",), outs=("raw", "act"))
fwd("tn.row.2048", "bf16", (1, 28, 256, 64, 2048, 3, 1, 1, 1), L, [("fwd.tn_group.row", "8")], "row kernel, eight N tiles: groups of four", tn_group=4,
    ops=("pre", "mask"), outs=("raw", "act"))

# ---- persistent grid with a ragged last round: 320 tiles on min(320, CUs) workgroups -- the name is the same on any CU count,
# only the walk differs (one tile more for some workgroups wherever the CU count does not divide 320)
for nops, ops_ in ((0, ()), (1, ("mask",)), (2, ("pre", "post"))):
    fwd(f"grid.row.320.{nops}", "bf16", (1, 320, 256, 64, 256, 3, 1, 2, 2), L, [("fwd.grid.row", f"ragged{nops}")],
        f"320 tiles on the lone-wave row kernel with {nops} epilogue operand(s): the next tile's first stages are issued before this epilogue",
        ops=ops_, outs=("raw", "act"))
    fwd(f"grid.1x1.320.{nops}", "bf16", (1, 160, 512, 64, 256, 1, 1, 0, 1), P, [("fwd.grid.1x1", f"ragged{nops}")],
        f"320 tiles on the ping-pong 1x1 kernel with {nops} epilogue operand(s)", ops=ops_, outs=("raw", "act"))

# ---- the entry points and epilogues that note a name of their own
fwd("dual", "bf16", (1, 224, 256, 64, 256, 1, 1, 0, 1), "conv_igemm_persist_kernel<pp,dual>", [("fwd.dual", "on")],
    "K-concatenated 1x1 conv (kd_conv1x1_dual_fwd): 64 + 64 channels from two sources in one accumulator chain", cin2=64, ops=("post",), outs=("raw", "act"))
fwd("cls", "bf16", (1, 224, 256, 64, 256, 3, 1, 1, 1), L, [("fwd.cls", "on")],
    "the classifier epilogue (19 classes) on the lone-wave row kernel: kd_conv2d_cls_supported must predict the kernel that is launched", cls=19, outs=())
fwd("out_sums", "bf16", (1, 224, 256, 64, 256, 1, 1, 0, 1), P, [("fwd.out_sums", "on")],
    "output sums without operands on the ping-pong 1x1 kernel: kd_conv2d_bn_sums_rows must predict the kernel that is launched", sums="out")

# ---- conv2d as the input gradient (KD_PACK_DGRAD weight): the dispatcher sees Cout -> Cin
dgrad("row", "bf16", (1, 224, 256, 256, 64, 3, 1, 2, 2), L, [("fwd.dgrad", "row")],
      "input gradient of a 256 -> 64 layer with dil 2: a 64 -> 256 conv to the dispatcher, lone-wave row kernel, ReLU mask + BN scale + shortcut gradient",
      ops=("mask", "post"), outs=("raw",))
dgrad("1x1", "bf16", (1, 224, 256, 256, 64, 1, 1, 0, 1), P, [("fwd.dgrad", "1x1")], "input gradient of a 1x1 256 -> 64 layer: ping-pong 1x1 kernel", ops=("mask",), outs=("raw",))
dgrad("narrow", "f32", (2, 6, 40, 64, 32, 3, 1, 3, 3), FN, [("fwd.dgrad", "narrow")], "fp32 input gradient of a small dilated layer: flipped taps on the gather kernel",
      ops=("mask",), outs=("raw",))

# =================================================================================================== weight-gradient table
WL, WR, WT, WW, WP = "conv_wgrad_lw_kernel", "conv_wgrad_row_kernel", "pw_wgrad_tr_kernel", "conv_wgrad_wide_kernel", "conv_wgrad_pw_lw_kernel"
WB, WF = "pw_wgrad_kernel<bf16>", "pw_wgrad_kernel<f32>"

wgrad("row.cout128", "bf16", (1, 4, 64, 64, 128, 3, 1, 1, 1), WL, [("wgrad.row.Cout%128", "128"), ("wgrad.row.W%64", "64"), ("wgrad.plan.stages", "under8,row")],
      "Cout = 128, dil 1, W = 64: lone-wave row kernel, four stages in one split")
wgrad("row.cout136", "bf16", (1, 4, 64, 64, 136, 3, 1, 1, 1), WR, [("wgrad.row.Cout%128", "136")], "Cout = 136: ragged second Cout tile -> the 8-wave row kernel", ldy_pad=8)
wgrad("row.dil8", "bf16", (1, 16, 64, 64, 128, 3, 1, 8, 8), WL, [("wgrad.row.dil<=8", "8")], "dil = 8: the last dilation of the lone-wave row kernel, H = 2 dil")
wgrad("row.dil9", "bf16", (1, 18, 64, 64, 128, 3, 1, 9, 9), WR, [("wgrad.row.dil<=8", "9")], "dil = 9: the 8-wave row kernel")
wgrad("row.dil16", "bf16", (1, 32, 64, 64, 128, 3, 1, 16, 16), WR, [("wgrad.row.WR_XROWS", "at")], "dil = 16: 64 + 2 * 16 = WR_XROWS rows, the buffer is full")
wgrad("row.dil17.small", "bf16", (1, 34, 64, 64, 128, 3, 1, 17, 17), WT, [("wgrad.row.WR_XROWS", "past,small"), ("wgrad.generic", "tr")],
      "dil = 17: past the row buffer, under 256 channels -> the transposing gather kernel, nine taps")
wgrad("row.dil17.wide", "bf16", (1, 8, 64, 256, 256, 3, 1, 17, 17), WW, [("wgrad.row.WR_XROWS", "past,wide"), ("wgrad.wide.geom", "3x3")],
      "dil = 17 with 256 x 256 channels: the wide tile with the general (gathered) staging; H < dil, so only the centre kernel row meets the image")
wgrad("row.w72", "bf16", (1, 4, 72, 64, 128, 3, 1, 1, 1), WT, [("wgrad.row.W%64", "72")], "W = 72: stages are not row segments -> gather kernel")
wgrad("row.f32", "f32", (1, 4, 64, 32, 128, 3, 1, 1, 1), WF, [("wgrad.row.bf16", "f32"), ("wgrad.generic", "f32")], "fp32 on the row shape: the fp32 generic kernel")
wgrad("wide.cin248", "bf16", (1, 8, 24, 248, 256, 1, 1, 0, 1), WT, [("wgrad.wide.Cin>=256", "248")], "Cin = 248 < 256: not wide, two ragged Cin tiles of the gather kernel")
wgrad("wide.cin256", "bf16", (1, 8, 24, 256, 256, 1, 1, 0, 1), WP, [("wgrad.wide.Cin>=256", "256"), ("wgrad.wide.Cout>=256", "256"), ("wgrad.pw_lw.M%64", "on"), ("wgrad.wide.geom", "1x1"),
                                                                  ("wgrad.reduce.n%4", "on")],
      "256 x 256 channels, 192 pixels: the lone-wave 1x1 kernel, three stages")
wgrad("wide.cout248", "bf16", (1, 8, 24, 256, 248, 1, 1, 0, 1), WT, [("wgrad.wide.Cout>=256", "248")], "Cout = 248 < 256: not wide")
wgrad("wide.m%64", "bf16", (1, 8, 25, 256, 256, 1, 1, 0, 1), WW, [("wgrad.pw_lw.M%64", "off")], "200 pixels: M % 64 != 0 -> the 8-wave wide kernel masks the last stage")
wgrad("wide.inside135", "bf16", (1, 8, 24, 304, 256, 1, 1, 0, 1), WW, [("wgrad.wide.135%", "inside")],
      "304 -> 256: 2 tiles of 256 x 256 against 6 of 128 x 128 is 133 % -- inside the 135 % rule (the layer the source's comment names); ragged second Cin tile")
wgrad("wide.outside135", "bf16", (1, 8, 24, 304, 304, 1, 1, 0, 1), WT, [("wgrad.wide.135%", "outside")],
      "304 -> 304: 4 tiles of 256 x 256 against 9 of 128 x 128 is 178 % -- outside, nine 128-tiles of the gather kernel")
wgrad("wide.cin%8", "bf16", (1, 8, 24, 260, 256, 1, 1, 0, 1), WB, [("wgrad.wide.Cin%8", "off"), ("wgrad.generic", "bf16")],
      "Cin = 260 through a padded view: Cin % 8 != 0 -> neither wide nor transposing, the scalar-load bf16 kernel", ldx_pad=12)
wgrad("gen.cout19", "bf16", (1, 7, 9, 65, 19, 1, 1, 0, 1), WB, [("wgrad.reduce.n%4", "off")],
      "19 x 65 = 1235 weights: the scalar arm of launch_slab_reduce (n % 4 != 0), operands through padded views", ldx_pad=15, ldy_pad=13)
wgrad("plan.one_stage", "bf16", (1, 1, 64, 64, 64, 1, 1, 0, 1), WT, [("wgrad.plan.stages", "one")], "64 pixels: one stage, one split")
wgrad("plan.under4", "bf16", (1, 3, 64, 64, 64, 1, 1, 0, 1), WT, [("wgrad.plan.stages", "under4")], "192 pixels: three stages, fewer than the four a split is kept to -> one split")
wgrad("plan.one_stage.row", "bf16", (1, 1, 64, 64, 128, 3, 1, 1, 1), WL, [("wgrad.plan.stages", "one,row")],
      "one image row of 64 pixels: one stage on the lone-wave row kernel, kernel rows 0 and 2 never meet the image")
wgrad("plan.cap768.tr", "bf16", (1, 384, 1024, 64, 64, 1, 1, 0, 1), WT, [("wgrad.plan.cap768", "tr")],
      "393216 pixels on one 128 x 128 tile: plan() asks 1024 splits, above the 768 the wide clause of the workspace bound is capped at; the bound must come from plan()")
wgrad("plan.cap768.wide", "bf16", (1, 384, 1024, 256, 256, 1, 1, 0, 1), WP, [("wgrad.plan.cap768", "wide")],
      "393216 pixels on one 256 x 256 tile: ceil(stages / 8) = 768 reaches the cap of the bound; fill_splits takes 256 splits of 24 stages")

pw("tr", "bf16", (1, 8, 24, 64, 128), WT, [("pw.generic", "tr")], "kd_pw_wgrad, under 256 channels: the transposing kernel")
pw("bf16.cout19", "bf16", (1, 8, 24, 64, 19), WB, [("pw.generic", "bf16")], "Cout = 19 through a padded view of dy: the scalar-load bf16 kernel", ldy_pad=13)
pw("f32", "f32", (1, 8, 24, 65, 19), WF, [("pw.generic", "f32")], "fp32, 19 x 65: the fp32 kernel and the scalar arm of the reduce", ldx_pad=15, ldy_pad=13)
pw("cin248", "bf16", (1, 8, 24, 248, 256), WT, [("pw.wide.Cin>=256", "248")], "kd_pw_wgrad, Cin = 248: not wide")
pw("cin256", "bf16", (1, 8, 24, 256, 256), WP, [("pw.wide.Cin>=256", "256"), ("pw.pw_lw.M%64", "on")], "kd_pw_wgrad, 256 x 256, 192 pixels: lone-wave kernel")
pw("m%64", "bf16", (1, 8, 25, 256, 256), WW, [("pw.pw_lw.M%64", "off")], "kd_pw_wgrad, 200 pixels: the 8-wave wide kernel")
pw("inside135", "bf16", (1, 8, 24, 256, 304), WW, [("pw.wide.135%", "inside")], "kd_pw_wgrad, 256 -> 304: 133 %, wide with a ragged second Cout tile")
pw("outside135", "bf16", (1, 8, 24, 264, 264), WT, [("pw.wide.135%", "outside")], "kd_pw_wgrad, 264 -> 264: 178 %, the transposing kernel")
