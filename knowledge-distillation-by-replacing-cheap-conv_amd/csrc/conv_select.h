// Which kernel kd_conv2d_fwd (conv_igemm.hip) and kd_conv2d_wgrad / kd_pw_wgrad (pw_wgrad.hip) run for a problem, and with what
// tiles, grid and epilogue variant: pure functions of the problem, the CU count and the A/B switches.  The launchers switch over
// the result and the queries of the ABI (kd_conv2d_bn_sums_rows, kd_conv2d_cls_supported, kd_conv1x1_dual_supported, the two
// workspace bounds) read its fields, so a query cannot disagree with the launch.  No HIP and no getenv here: a plain host C++
// compiler accepts this file, and tests/test_conv_select_host.py holds it against the restatement of tests/_conv_dispatch_cases.py.
#pragma once
#include <stdint.h>

#include "../../include/kdcc.h"

// ---- forward / input gradient ----------------------------------------------------------------------------------------------
// One value per name the launcher notes in the kernel-selection log.
enum ConvKernel {
    CONV_ROW_DUO, CONV_ROW_PERSIST_DBG, CONV_ROW_LW, CONV_ROW_PERSIST_PP, CONV_ROW_PERSIST_LOCKSTEP,
    CONV_PW_LW, CONV_IGEMM_PERSIST_PP_DUAL, CONV_IGEMM_PERSIST_PP, CONV_IGEMM_PERSIST_LOCKSTEP,
    CONV_ROW_HALF, CONV_ROW_TALL, CONV_ROW_PP128,
    CONV_ROW_NARROW, CONV_ROW_F32_X, CONV_ROW_X, CONV_ROW_F32_WIDE, CONV_ROW_WIDE,
    CONV_IGEMM_HALF, CONV_IGEMM_WIDE, CONV_IGEMM_DEEP, CONV_IGEMM_NARROW, CONV_IGEMM_NARROW2,
    CONV_IGEMM_F32_WIDE, CONV_IGEMM_F32_DEEP, CONV_IGEMM_F32_NARROW,
};
enum ConvCfgSwitch { CONV_CFG_DEFAULT, CONV_CFG_NARROW, CONV_CFG_NOROW, CONV_CFG_HALF, CONV_CFG_DEEP, CONV_CFG_NARROW1 };   // KDCC_CONV_CFG

// Every KDCC_* switch conv_igemm.hip reads (conv_switches() there builds it once per process); the defaults are the shipped configuration.
struct ConvSwitches {
    int lw = 1;            // KDCC_CONV_LW: conv_row_lw_kernel / conv_row_tall_kernel (one wave per SIMD, hand-scheduled loop); 0 = the 8-wave kernels
    int pp = 1;            // KDCC_CONV_PP: 0 = lock-step waves
    int persist = 1;       // KDCC_CONV_PERSIST: 0 = one tile per workgroup
    int cfg = CONV_CFG_DEFAULT;
    int duo = 0;           // KDCC_CONV_DUO: 0 off, 1 the Cout = 128 layers (instead of the 512 x 128 ping-pong kernel), 2 every row-buffer layer it fits
    int lw_pw = 0;         // KDCC_CONV_LW_PW: 1 = conv_pw_lw_kernel on the 1x1 layers
    int tngroup = 4;       // KDCC_CONV_TNGROUP
    int dual = 1;          // KDCC_CONV_DUAL: 0 = two launches (engine falls back)
    int epi_batch = 1;     // KDCC_EPI_BATCH: 0 = one pass at a time
    int persist_cus = 0;   // KDCC_PERSIST_CUS (kd_conv_set_persist_cus overrides it)
    int tune = 0, stagger_us = 0;   // KDCC_CONV_TUNE, KDCC_CONV_STAGGER: timing ablations / timestamps, tuning build only
};

// (N tile, bytes of K per stage, last dilation of the row buffer) of the tile configurations; conv_igemm.hip asserts them against its Cfg types
struct ConvTile { int bn, rb; };
constexpr ConvTile CONV_TILE_128{128, 128}, CONV_TILE_256{256, 128}, CONV_TILE_256_K64{256, 64}, CONV_TILE_128_K64{128, 64};
constexpr int CONV_ROW_MAXDIL = 32, CONV_ROWX_MAXDIL = 64, CONV_ROWN_MAXDIL = 64;
struct ConvSel {
    ConvKernel kernel;
    int epi;               // epilogue variant: the NOPS template argument, or the nops_sums argument of the conv_lw.hip launchers
    bool row_x, plain;     // the 384-row buffer (dil > 32); KDCC_CONV_TUNE & 8: the plain main loop on the wide gather tiles
    int vec_ok, nops;      // every epilogue pointer / stride 16-B friendly; epilogue operands
    int nkc, nk, nk1;      // K stages per tap, in all, and of the first source (K-concatenated 1x1)
    int tiles_m, tiles_n, ntiles, tn_group;
    int wg_per_cu;         // grid rule: 0 = one workgroup per tile, else a persistent grid of this many workgroups per CU (conv_grid)
    int sums_rows;         // rows of ep->bn_sums partials the kernel writes when asked (kd_conv2d_bn_sums_rows), 0 = it does not
    bool cls_ok, dual_ok;  // the classifier epilogue / the second A source (cin1 > 0) are granted
};

// Workgroups per "one per CU" of the persistent grids: every CU (n == 0), or fewer (a multiple of 8, one XCD round) when KDCC_PERSIST_CUS / kd_conv_set_persist_cus says so
static inline int conv_persist_cus(int n, int ncu)
{
    if (n <= 0 || n > ncu) n = ncu;        // 0 = every CU; a cap above the CU count is the full chip
    if (n < 8) n = 8;                      // a cap below one XCD round is one XCD round (never "the full chip")
    return n - n % 8;
}
static inline unsigned conv_grid(const ConvSel &c, int persist_cus)
{
    if (!c.wg_per_cu) return (unsigned)c.ntiles;
    const int cap = c.wg_per_cu * persist_cus, nwg = c.ntiles < cap ? c.ntiles : cap;
    return (unsigned)((nwg + 7) / 8 * 8);
}

// cin1 > 0: K-concatenated 1x1 conv (kd_conv1x1_dual_fwd) -- d->Cin is the TOTAL reduction depth, channels [0, cin1) come from the first source
static inline ConvSel conv_select(const kd_conv_desc *d, const kd_conv_epilogue *ep, int cin1, int ncu, const ConvSwitches &sw)
{
    ConvSel c{};
    const bool bf16 = d->dtype == KD_BF16, lw_row = sw.lw != 0, pp_row = sw.pp != 0, dbg = (sw.tune & 512) != 0, sums = ep->bn_sums != nullptr;
    const int es = bf16 ? 2 : 4, M = d->N * d->Ho * d->Wo;
    auto ok = [&](const void *ptr, int ld, int esz) { return !ptr || (((uintptr_t)ptr & 15u) == 0 && (ld * esz) % 16 == 0); };
    c.vec_ok = ok(ep->res_pre, ep->ld_res_pre, es) && ok(ep->mask, ep->ld_mask, es) && ok(ep->res_post, ep->ld_res_post, es) &&
               ok(ep->out_raw, ep->ld_raw, ep->raw_f32 ? 4 : es) && ok(ep->out_act, ep->ld_act, es);
    const int nops = c.nops = (ep->res_pre ? 1 : 0) + (ep->mask ? 1 : 0) + (ep->res_post ? 1 : 0);
    // wide tiles only when they still fill the chip (one workgroup per CU, 256 CUs); e.g. the ASPP 4096->256 1x1 at
    // 128x256 pixels would give 128 wide tiles, so it runs on the narrow config (256 tiles)
    const long long wide_tiles = (long long)((M + 255) / 256) * ((d->Cout + CONV_TILE_256.bn - 1) / CONV_TILE_256.bn);
    int cfg = (d->Cout > 128 && wide_tiles >= 224) ? 1 : 0;   // 0 narrow2, 1 wide, 2 deep, 3 narrow (one workgroup per CU)
    if (sw.cfg == CONV_CFG_NARROW) cfg = 0;                    // tuning hook
    else if (sw.cfg == CONV_CFG_DEEP && cfg == 1) cfg = 2;
    else if (sw.cfg == CONV_CFG_NARROW1 && cfg == 0) cfg = 3;
    const bool norow = sw.cfg == CONV_CFG_NOROW, half = sw.cfg == CONV_CFG_HALF;
    // 256-pixel tiles that are segments of one image row, 3x3 / stride 1 / 'same': row-buffer kernels (the narrow one is
    // compiled for <= 128 VGPRs, which the fp32 parity path's blocked accumulation does not fit)
    const bool row_geom = !norow && d->kh == 3 && d->kw == 3 && d->stride == 1 && d->pad == d->dil && d->W % 256 == 0;
    const bool row_wide = row_geom && cfg == 1 && d->dil <= CONV_ROWX_MAXDIL;
    const bool row_x = c.row_x = row_wide && d->dil > CONV_ROW_MAXDIL;
    const bool row_narrow = row_geom && cfg == 0 && bf16 && d->dil <= CONV_ROWN_MAXDIL;
    // persistent kernels (bf16 wide tiles, whole tiles, vector-friendly epilogue): one workgroup per CU walks the tiles
    const bool persist_ok = sw.persist && !half && bf16 && cfg == 1 && c.vec_ok && !ep->raw_f32 && M % 256 == 0 && d->Cout % 256 == 0 &&
                            (nops <= 2 || (pp_row && !dbg));   // three operands: the default (ping-pong) instantiations only
    const bool use_row_persist = persist_ok && row_wide && !row_x;
    const bool use_igemm_persist = !use_row_persist && persist_ok && d->kh == 1 && d->stride == 1 && d->pad == 0;
    const bool use_pp128 = !use_row_persist && !use_igemm_persist && !(row_wide && half && bf16) && row_narrow && pp_row && sw.persist &&
                           c.vec_ok && !ep->raw_f32 && nops <= 2 && d->Cout % 128 == 0 && d->W % 512 == 0 && d->dil <= 16 && d->Cin % 32 == 0;
    // conv_row_duo_kernel (conv_lw.hip): 256 x 128 tiles, two workgroups per CU -- one's epilogue under the other's main loop.
    // H >= 2 dil: every output row has >= 2 kernel rows inside the image, which the lone-wave loops' period hand-over assumes (with
    // dil < H < 2 dil the rows H - dil <= ho < dil have one; they go to the ping-pong kernel, which counts kernel rows per tile)
    const bool lone_wave_row = lw_row && bf16 && d->kh == 3 && d->kw == 3 && d->stride == 1 && d->pad == d->dil && d->dil <= 32 && d->H >= 2 * d->dil && !dbg;
    const bool duo_ok = sw.duo > 0 && lone_wave_row && d->W % 256 == 0 && M % 256 == 0 && d->Cout % 128 == 0 && d->Cin % 64 == 0 && c.vec_ok &&
                        !ep->raw_f32 && nops <= 1 && !sums && (long long)(M / 256) * (d->Cout / 128) >= 2 * ncu && (sw.duo >= 2 || d->Cout == 128);
    // the sums: with a mask, the ping-pong instantiations with one or two epilogue operands (with three the sums' registers spill
    // 150 values); without, the sums of the OUTPUT (S1 = sum of the stored values, S2 = 0), which only the ping-pong 1x1 kernel
    // without epilogue operands and with the raw output alone takes (the tensor the ASPP image pooling averages)
    const bool sums_ok = pp_row && !dbg &&
                         (ep->mask ? (use_row_persist || use_igemm_persist || use_pp128) && !(use_row_persist && d->dil > 32) && nops <= 2
                                   : use_igemm_persist && nops == 0 && ep->out_raw && !ep->out_act && !ep->raw_f32 && !sw.lw_pw);
    c.sums_rows = sums_ok ? (int)((long long)d->N * d->Ho * d->Wo / 128) : 0;
    // epilogue variants: nops | 4 = with the mask sums, 8 = the output sums alone (1x1 only); the lock-step and phase-clock forms take <= 2 operands
    const int pp_epi = (sums && nops >= 1 && nops <= 2) ? (nops | 4) : nops, two_epi = nops < 2 ? nops : 2, lw_epi = nops | (sums ? 4 : 0);
    int bm = 256;   // pixels and (channels, K bytes) of a tile
    ConvTile t = CONV_TILE_256;
    if (duo_ok) {
        c.kernel = CONV_ROW_DUO; c.epi = nops; t = CONV_TILE_128_K64; c.wg_per_cu = 2;
    } else if (use_row_persist) {
        const bool lw = lone_wave_row && pp_row;
        c.kernel = dbg ? CONV_ROW_PERSIST_DBG : lw ? CONV_ROW_LW : (pp_row && d->dil <= 32) ? CONV_ROW_PERSIST_PP : CONV_ROW_PERSIST_LOCKSTEP;
        c.epi = c.kernel == CONV_ROW_LW ? ((ep->cls_w || ep->cls_out) ? 16 : lw_epi) : c.kernel == CONV_ROW_PERSIST_PP ? pp_epi : two_epi;
        c.wg_per_cu = 1;
    } else if (use_igemm_persist) {
        // conv_pw_lw_kernel (the lone-wave loop for 1x1 layers) is bit-identical but NOT faster here: its main loop ties the
        // ping-pong kernel's (8 DMA pieces per k-step keep both near the staging rate) and its serial epilogue -- four waves with
        // twice the instructions each, nothing to overlap them -- costs 10-60 % more on these short-K layers (tools/lw_ablate.sh).
        const bool lw = sw.lw_pw && lw_row && pp_row && d->Cin % 128 == 0 && !dbg && !cin1;
        c.kernel = lw ? CONV_PW_LW : !pp_row ? CONV_IGEMM_PERSIST_LOCKSTEP : cin1 ? CONV_IGEMM_PERSIST_PP_DUAL : CONV_IGEMM_PERSIST_PP;
        c.epi = lw ? lw_epi : !pp_row ? two_epi : (sums && nops == 0) ? 8 : pp_epi;
        c.wg_per_cu = 1;
    } else if (row_wide && half && bf16) {
        c.kernel = CONV_ROW_HALF; t = CONV_TILE_128_K64;
    } else if (use_pp128) {
        // Cout = 128 layers: 512 x 128 ping-pong tiles.  conv_row_tall_kernel (conv_lw.hip): the same tiles with one wave per SIMD
        // and the hand-scheduled loop
        const bool tall = lw_row && d->Cin % 64 == 0 && d->H > d->dil && !dbg && !(sums && nops == 0);
        c.kernel = tall ? CONV_ROW_TALL : CONV_ROW_PP128;
        c.epi = tall ? lw_epi : dbg ? -1 : pp_epi;   // (-1: phase clocks, the no-operand form only)
        bm = 512; t = CONV_TILE_128_K64; c.wg_per_cu = 1;
    } else if (row_wide || row_narrow) {
        c.kernel = row_narrow ? CONV_ROW_NARROW : row_x ? (bf16 ? CONV_ROW_X : CONV_ROW_F32_X) : (bf16 ? CONV_ROW_WIDE : CONV_ROW_F32_WIDE);
        if (row_narrow) t = CONV_TILE_128_K64;
    } else if (bf16) {
        c.kernel = cfg == 1 ? (half ? CONV_IGEMM_HALF : CONV_IGEMM_WIDE) : cfg == 2 ? CONV_IGEMM_DEEP : cfg == 3 ? CONV_IGEMM_NARROW : CONV_IGEMM_NARROW2;
        c.plain = cfg == 1 && (sw.tune & 8);   // A/B: plain main loop
        t = c.plain ? CONV_TILE_256 : cfg == 1 ? (half ? CONV_TILE_128_K64 : CONV_TILE_256) : cfg == 2 ? CONV_TILE_256_K64 : cfg == 3 ? CONV_TILE_128 : CONV_TILE_128_K64;
    } else {   // fp32 parity path: its blocked accumulation does not fit 128 VGPRs
        c.kernel = cfg == 1 ? CONV_IGEMM_F32_WIDE : cfg == 2 ? CONV_IGEMM_F32_DEEP : CONV_IGEMM_F32_NARROW;
        t = cfg == 1 ? CONV_TILE_256 : cfg == 2 ? CONV_TILE_256_K64 : CONV_TILE_128;
    }
    c.nkc = d->Cin / (t.rb / es);
    c.nk = d->kh * d->kw * c.nkc;
    c.nk1 = c.kernel == CONV_IGEMM_PERSIST_PP_DUAL ? cin1 / (t.rb / es) : 0x7fffffff;
    c.tiles_m = (M + bm - 1) / bm;
    c.tiles_n = (d->Cout + t.bn - 1) / t.bn;
    c.ntiles = c.tiles_m * c.tiles_n;
    // N tiles walked four at a time over all M tiles (Cout >= 2048): an XCD then keeps 4 weight slabs (K x 256) in its L2 for
    // the whole launch instead of cycling all 8-16 of them per round of tiles; +3-4 % on the 4096-wide 1x1 layers.  (The duo
    // kernel's 8 tiles of 128 channels = 4 of 256; the 512 x 128 tiles are not grouped.)
    const int tng = (256 / t.bn) * sw.tngroup;
    c.tn_group = (c.wg_per_cu && bm == 256 && sw.tngroup > 0 && c.tiles_n > tng && c.tiles_n % tng == 0) ? tng : 0;
    c.cls_ok = c.kernel == CONV_ROW_LW && nops == 0 && sw.duo < 2;
    c.dual_ok = c.kernel == CONV_IGEMM_PERSIST_PP_DUAL && sw.dual && cin1 % (t.rb / es) == 0;
    return c;
}

// ---- weight gradient -------------------------------------------------------------------------------------------------------
enum WgradKernel { WGRAD_LW, WGRAD_ROW, WGRAD_PW_LW, WGRAD_WIDE, WGRAD_WIDE_GENERAL, WGRAD_TR, WGRAD_BF16, WGRAD_F32 };   // (WIDE_GENERAL: conv_wgrad_wide_kernel with the gathered staging)

// Every KDCC_* switch pw_wgrad.hip reads (wgrad_switches() there builds it once per process)
struct WgradSwitches {
    int row = 2;            // KDCC_WGRAD_ROW: 0 = never, 1 = only where the 256 x 256 tile is not chosen, 2 = wherever eligible (default: faster on every 3x3
                            // layer of the net, tools/bench_wgrad.py at 4 images: 128->128 1.70 -> 1.06 ms, 304->256 7.25 -> 4.69, 256->256 1.04 -> 0.88, 64->128 1.51 -> 0.83)
    int lw = 1;             // KDCC_WGRAD_LW: 0 = conv_wgrad_row_kernel (8 waves); bit-identical
    int wide = 1;           // KDCC_WGRAD_WIDE: 0 = never the 256 x 256 tile
    int wide_general = 0;   // KDCC_WGRAD_WIDE_GENERAL: the general staging on 1x1 too
    int pw_lw = 1;          // KDCC_WGRAD_PW_LW: 0 = conv_wgrad_wide_kernel (8 waves); bit-identical
    int target = 0, wide_target = 0;   // KDCC_WGRAD_TARGET, KDCC_WGRAD_WIDE_TARGET: floor(n / workgroups per split)
    int nst = 2;            // KDCC_WGRAD_NST: 2 | 3 | 4 (measured: 128->128 3x3 at 512x1024 1.70 ms with 2, 2.44 with 3 or 4: occupancy beats depth)
    int il = 1;             // KDCC_WGRAD_IL (tuning build): 0 = reads in front of the MFMAs, 1 = interleaved (shipped), 2 = ping-pong
    int dbg = 0;            // KDCC_WGRAD_DBG: phase clocks, tuning build only
};

struct WgradSel {
    WgradKernel kernel;
    int tiles, tiles_ci, splits, rps;
    unsigned grid[3];
};

constexpr int WR_XROWS = 96;   // row-buffer rows of conv_wgrad_row_kernel: 64 + 2 * dil <= 96

static inline void wgrad_plan(int dtype, int M, int Cin, int Cout, int taps, WgradSel &c)
{
    const int krows = 128 / (dtype == KD_BF16 ? 2 : 4);   // pixels per K stage
    c.tiles_ci = (Cin + 127) / 128;
    c.tiles = c.tiles_ci * ((Cout + 127) / 128);
    const int stages = (M + krows - 1) / krows;
    const int want = (1024 + c.tiles * taps - 1) / (c.tiles * taps);   // aim for ~1024 workgroups (4 per CU)
    const int max_splits = (stages + 3) / 4;                          // keep >= 4 stages per split
    c.splits = want > max_splits ? max_splits : want;
    if (c.splits < 1) c.splits = 1;
    c.rps = (stages + c.splits - 1) / c.splits * krows;
    c.splits = (M + c.rps - 1) / c.rps;
}

// Split-K factor for kernels that run ONE workgroup per CU, all of equal length (the 256 x 256 and the row-buffer weight-gradient
// tiles): the launch takes ceil(W / 256) rounds of the 256 CUs with W = splits * per workgroups, so W should sit just BELOW a
// multiple of 256, and the fewest rounds that fill the chip win (fewer partial slabs to write and reduce, fewer pipeline fills).
// Returns the first floor(256 k / per), k = 1..4, that fills >= 95 % of its k rounds, else the best fill.  Round 2 aimed at "about
// 640 / 768 workgroups" rounded UP: 2.5 rounds with the last half empty, or one workgroup into a fourth round.  Measured
// (tools/bench_wgrad.py, 4 images): 3x3 128->128 at 512x1024 1.01 -> 0.85 ms, 256->256 at 512x1024 2.99 -> 2.50, 512->512 0.78 -> 0.73,
// 1024->512 1.44 -> 1.27, 304->256 4.45 -> 3.87; 1x1 512->512 0.220 -> 0.114, 4096->256 0.371 -> 0.313; mode B 24.5 -> 25.8 img/s.
static inline int wgrad_fill_splits(int per, int max_splits)
{
    int splits = 1;
    double best = -1.0;
    for (int k = 1; k <= 4; ++k) {
        int sp = (256 * k) / per;
        sp = sp < 1 ? 1 : (sp > max_splits ? max_splits : sp);
        const long long w = (long long)sp * per;
        const double fill = (double)w / (double)(((w + 255) / 256) * 256);
        if (fill >= 0.95) return sp;
        if (fill > best) { best = fill; splits = sp; }
    }
    return splits;
}

// plan of the one-per-CU tiles, >= 8 stages of 64 pixels per split: the row-buffer kernel (tile = 128, three kernel rows per tile:
// ~2.5 workgroups per CU) and the 256 x 256 tile (bf16 LDS-DMA path, ~3 waves of workgroups)
static inline void wgrad_plan64(long long M, int Cin, int Cout, int tile, int per_tile, int stages, int target, WgradSel &c)
{
    c.tiles_ci = (Cin + tile - 1) / tile;
    c.tiles = c.tiles_ci * ((Cout + tile - 1) / tile);
    const int per = c.tiles * per_tile, max_splits = (stages + 7) / 8;
    c.splits = target > 0 ? target / per : wgrad_fill_splits(per, max_splits);
    c.splits = c.splits < 1 ? 1 : (c.splits > max_splits ? max_splits : c.splits);
    c.rps = ((stages + c.splits - 1) / c.splits) * 64;
    c.splits = (int)((M + c.rps - 1) / c.rps);
}
static inline bool wgrad_row_eligible(const kd_conv_desc *d)
{
    return d->dtype == KD_BF16 && d->kh == 3 && d->kw == 3 && d->stride == 1 && d->pad == d->dil && 2 * d->dil + 64 <= WR_XROWS &&
           d->W % 64 == 0 && d->Cin % 8 == 0 && d->Cout % 8 == 0;
}

// d: the conv (kd_conv2d_wgrad), or nullptr for kd_pw_wgrad -- one tap, no geometry; it takes neither the row kernel nor the
// general wide staging
static inline WgradSel wgrad_select(int dtype, long long M, int Cin, int Cout, int taps, const kd_conv_desc *d, const WgradSwitches &sw)
{
    WgradSel c{};
    const bool bf16 = dtype == KD_BF16;
    // the 256 x 256 tile (444 -> 624 TFLOP/s on large layers) where its padding pays
    const long long pad256 = (long long)((Cout + 255) / 256) * ((Cin + 255) / 256) * 65536;
    const long long pad128 = (long long)((Cout + 127) / 128) * ((Cin + 127) / 128) * 16384;
    const bool wide = sw.wide && bf16 && Cin % 8 == 0 && Cout % 8 == 0 && Cout >= 256 && Cin >= 256 &&
                      pad256 * 100 <= pad128 * 135;   // (the decoder's 304-channel conv: 2 x 256 vs 3 x 128 columns)
    const bool geom = d && !(taps == 1 && d->stride == 1 && d->pad == 0);
    c.grid[0] = c.grid[1] = c.grid[2] = 1;
    if (d && wgrad_row_eligible(d) && (sw.row == 2 || (sw.row == 1 && !wide))) {
        wgrad_plan64(M, Cin, Cout, 128, 3, (int)(M / 64), sw.target, c);
        // (Cin % 8 == 0: row_eligible; a ragged last Cin tile is masked)
        c.kernel = (sw.lw && !sw.dbg && d->Cout % 128 == 0 && d->dil <= 8) ? WGRAD_LW : WGRAD_ROW;
        c.grid[0] = (unsigned)(c.tiles * c.splits * 3);
        return c;
    }
    if (wide) {
        wgrad_plan64(M, Cin, Cout, 256, taps, (int)((M + 63) / 64), sw.wide_target, c);
        const bool general = geom || (d && sw.wide_general);
        // conv_wgrad_pw_lw_kernel instead of conv_wgrad_wide_kernel<true>: whole 256 x 256 tiles and whole 32-pixel stages.  Measured at 8 images
        // (tools/wgrad_lw_check.py, ms incl. the reduce): 2048->4096 4.49 -> 3.28, 1024->2048 1.19 -> 0.80, 2048->1024 1.17 -> 0.78, 4096->256 0.85 -> 0.66,
        // 512->1024 0.34 -> 0.22, 1280->256 0.24 -> 0.18, 512->512 0.20 -> 0.15.  (With the workgroups dealt round-robin over the XCDs, as the 8-wave
        // kernel's 2-D grid is, the short splits were SLOWER than the 8-wave kernel, x 0.90-0.92: the tiles of a split fetched their shared rows into
        // eight L2s.)
        const bool lw = !sw.dbg && !general && taps == 1 && sw.pw_lw && Cin % 256 == 0 && Cout % 256 == 0 && M % 64 == 0 && c.rps % 32 == 0;
        c.kernel = lw ? WGRAD_PW_LW : general ? WGRAD_WIDE_GENERAL : WGRAD_WIDE;
    } else {
        wgrad_plan(dtype, (int)M, Cin, Cout, taps, c);
        c.kernel = (bf16 && Cin % 8 == 0 && Cout % 8 == 0) ? WGRAD_TR : bf16 ? WGRAD_BF16 : WGRAD_F32;
    }
    if (c.kernel == WGRAD_PW_LW) c.grid[0] = (unsigned)(c.tiles * c.splits);
    else { c.grid[0] = (unsigned)c.tiles; c.grid[1] = (unsigned)c.splits; c.grid[2] = (unsigned)taps; }
    return c;
}

// Splits the workspace of a weight gradient is sized for (x taps x Cout x Cin floats): an upper bound over both dtypes and every
// plan above, not the need of the plan taken -- the generic plan with the smaller K stage (f32: 32 rows) gives the larger split count
static inline int wgrad_workspace_splits(int M, int Cin, int Cout, int taps, const kd_conv_desc *d, const WgradSwitches &sw)
{
    WgradSel c{};
    wgrad_plan(KD_F32, M, Cin, Cout, taps, c);
    int splits = c.splits;
    wgrad_plan(KD_BF16, M, Cin, Cout, taps, c);
    if (c.splits > splits) splits = c.splits;
    const int stages = (M + 63) / 64;
    const int wsplits = (stages + 7) / 8 < 768 ? (stages + 7) / 8 : 768;   // the wide-tile plan never splits finer
    if (wsplits > splits) splits = wsplits;
    if (d && wgrad_row_eligible(d)) {
        wgrad_plan64(M, Cin, Cout, 128, 3, (int)(M / 64), sw.target, c);
        if (c.splits > splits) splits = c.splits;
    }
    return splits;
}
