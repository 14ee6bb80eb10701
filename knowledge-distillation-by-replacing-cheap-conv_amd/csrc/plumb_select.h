// Which kernel the trunk, backward and small-shape plumbing entry points (trunk_ops.hip, bwd_ops.hip, small_ops.hip) run for a
// call, on what grids and with what plan: a pure function of the shape, the dtypes and the operands' pointer values and leading
// dimensions.  The launchers check their arguments, call the selector of their entry point, note plumb_kernel_name(sel.kernel) and
// switch over sel.kernel; the workspace queries return the functions below.  No HIP, no getenv and no globals here: a plain host
// C++ compiler accepts this file, and tests/test_plumb_select_host.py holds it against tests/_plumbing_cases.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/kdcc.h"
#include "resample.h"

// One value per name the launchers note (plumb_kernel_name), then PLUMB_REFUSED.  Where a kernel has dtype / vector variants they
// are a range in the order <f32 before bf16> x <scalar before vector>, the first operand's dtype slowest.
enum PlumbKernel {
    PK_STEM_CONV_F32, PK_STEM_CONV_MFMA, PK_STEM_POOL,
    PK_MAXPOOL_F32, PK_MAXPOOL_BF16,
    PK_UP_F32_F32_1, PK_UP_F32_F32_8, PK_UP_F32_BF16_1, PK_UP_F32_BF16_8,           // PK_UP_F32_F32_1 + 4 * (x is bf16) + 2 * (y is bf16) + vec
    PK_UP_BF16_F32_1, PK_UP_BF16_F32_8, PK_UP_BF16_BF16_1, PK_UP_BF16_BF16_8,
    PK_UP_FLAT4_F32, PK_UP_FLAT4_BF16,
    PK_GAP_PARTIAL_F32, PK_GAP_PARTIAL_BF16,
    PK_BN_FOLD, PK_COPY_CAST_CFAST, PK_COPY_CAST_PFAST,
    PK_RELU_BN_BWD_F32, PK_RELU_BN_BWD_BF16,
    PK_CS_F32_1, PK_CS_F32_8, PK_CS_BF16_1, PK_CS_BF16_8,                           // PK_CS_F32_1 + 2 * bf16 + vec
    PK_BNS_STAGE_64, PK_BNS_STAGE_256, PK_CS_FINISH,
    PK_BN_EVAL_PARAM_GRADS,
    PK_MP_ARGMAX_F32, PK_MP_ARGMAX_BF16,
    PK_MPB_F32_1, PK_MPB_F32_8, PK_MPB_BF16_1, PK_MPB_BF16_8,                       // PK_MPB_F32_1 + 2 * bf16 + vec
    PK_UPB_F32_F32_1, PK_UPB_F32_F32_8, PK_UPB_F32_BF16_1, PK_UPB_F32_BF16_8,       // PK_UPB_F32_F32_1 + 4 * (gy is bf16) + 2 * (gx is bf16) + vec
    PK_UPB_BF16_F32_1, PK_UPB_BF16_F32_8, PK_UPB_BF16_BF16_1, PK_UPB_BF16_BF16_8,
    PK_ZERO_INSERT_F32, PK_ZERO_INSERT_BF16,
    PK_BCAST_ADD_F32, PK_BCAST_ADD_BF16,
    PK_STEM_WGRAD_MFMA, PK_STEM_WGRAD_F32, PK_STEM_WGRAD_BF16,
    PK_DCONV_WGRAD,
    PK_BN2D_FWD_EVAL, PK_BN2D_FWD_TRAIN, PK_BN2D_BWD_EVAL, PK_BN2D_BWD_TRAIN,
    PLUMB_REFUSED,   // not a kernel: the call is outside what the entry point's kernels take
};
static inline const char *plumb_kernel_name(int k)
{
    static const char *const names[] = {
        "stem_conv_kernel<f32>", "stem_conv_mfma_kernel", "stem_pool_kernel",
        "maxpool_kernel<f32>", "maxpool_kernel<bf16>",
        "upsample_kernel<f32,f32,1>", "upsample_kernel<f32,f32,8>", "upsample_kernel<f32,bf16,1>", "upsample_kernel<f32,bf16,8>",
        "upsample_kernel<bf16,f32,1>", "upsample_kernel<bf16,f32,8>", "upsample_kernel<bf16,bf16,1>", "upsample_kernel<bf16,bf16,8>",
        "upsample_flat4_kernel<f32>", "upsample_flat4_kernel<bf16>",
        "gap_partial_kernel<f32>", "gap_partial_kernel<bf16>",
        "bn_fold_kernel", "copy_cast_kernel<c_fast>", "copy_cast_kernel<p_fast>",
        "relu_bn_bwd_kernel<f32>", "relu_bn_bwd_kernel<bf16>",
        "channel_sums_partial_kernel<f32,1>", "channel_sums_partial_kernel<f32,8>", "channel_sums_partial_kernel<bf16,1>", "channel_sums_partial_kernel<bf16,8>",
        "bn_sums_stage_kernel<64 rows>", "bn_sums_stage_kernel<256 rows>", "channel_sums_finish_kernel",
        "bn_eval_param_grads_kernel",
        "maxpool_argmax_kernel<f32>", "maxpool_argmax_kernel<bf16>",
        "maxpool_bwd_kernel<f32,1>", "maxpool_bwd_kernel<f32,8>", "maxpool_bwd_kernel<bf16,1>", "maxpool_bwd_kernel<bf16,8>",
        "upsample_bwd_kernel<f32,f32,1>", "upsample_bwd_kernel<f32,f32,8>", "upsample_bwd_kernel<f32,bf16,1>", "upsample_bwd_kernel<f32,bf16,8>",
        "upsample_bwd_kernel<bf16,f32,1>", "upsample_bwd_kernel<bf16,f32,8>", "upsample_bwd_kernel<bf16,bf16,1>", "upsample_bwd_kernel<bf16,bf16,8>",
        "zero_insert_kernel<f32>", "zero_insert_kernel<bf16>",
        "broadcast_add_kernel<f32>", "broadcast_add_kernel<bf16>",
        "stem_wgrad_mfma_kernel", "stem_wgrad_kernel<f32>", "stem_wgrad_kernel<bf16>",
        "dconv_wgrad_kernel",
        "bn2d_fwd_kernel<eval>", "bn2d_fwd_kernel<train>", "bn2d_bwd_kernel<eval>", "bn2d_bwd_kernel<train>"};
    static_assert(sizeof(names) / sizeof(names[0]) == PLUMB_REFUSED, "one name per kernel value");
    return k >= 0 && k < PLUMB_REFUSED ? names[k] : nullptr;
}
static_assert(PK_MAXPOOL_BF16 == PK_MAXPOOL_F32 + 1 && PK_UP_BF16_BF16_8 == PK_UP_F32_F32_1 + 7 && PK_UP_F32_BF16_1 == PK_UP_F32_F32_1 + 2 &&
              PK_UP_FLAT4_BF16 == PK_UP_FLAT4_F32 + 1 && PK_GAP_PARTIAL_BF16 == PK_GAP_PARTIAL_F32 + 1 && PK_RELU_BN_BWD_BF16 == PK_RELU_BN_BWD_F32 + 1 &&
              PK_CS_BF16_8 == PK_CS_F32_1 + 3 && PK_MP_ARGMAX_BF16 == PK_MP_ARGMAX_F32 + 1 && PK_MPB_BF16_8 == PK_MPB_F32_1 + 3 &&
              PK_UPB_BF16_BF16_8 == PK_UPB_F32_F32_1 + 7 && PK_UPB_F32_BF16_1 == PK_UPB_F32_F32_1 + 2 && PK_ZERO_INSERT_BF16 == PK_ZERO_INSERT_F32 + 1 &&
              PK_BCAST_ADD_BF16 == PK_BCAST_ADD_F32 + 1 && PK_STEM_WGRAD_BF16 == PK_STEM_WGRAD_F32 + 1 && PK_BN2D_FWD_TRAIN == PK_BN2D_FWD_EVAL + 1 &&
              PK_BN2D_BWD_TRAIN == PK_BN2D_BWD_EVAL + 1 && KD_F32 == 0 && KD_BF16 == 1,
              "the selectors compute the dtype / vector variants from the order of PlumbKernel");

// What the kernels' translation units are built for; they alias these or static_assert against them.
constexpr int PLUMB_SW_SEG = 256;               // columns of a stem_wgrad work item (one image row segment)
constexpr int PLUMB_STEM_MAX_BLOCKS = 768;      // stem_wgrad: three 256-thread blocks per CU (41 KiB of LDS each): one round
constexpr int PLUMB_STEM_MFMA_MAX_BLOCKS = 256 * 16;   // stem_conv_mfma_kernel: persistent-ish, 16 workgroups per CU
constexpr int PLUMB_SP_COLS = 7, PLUMB_SP_ROWS = 16;   // stem_pool_kernel: pooled columns per wave, pooled rows per wave segment
constexpr int PLUMB_GAP_CHUNKS = 64;            // pixel chunks of an image in gap_partial_kernel
constexpr int PLUMB_UP_RO = 8;                  // output rows a thread of the upsample kernels produces
// kd_channel_sums: >= 512 rows (64 per thread) per block, at most 1024 chunks; ~2048 blocks over (groups, channel blocks, chunks)
// fill the chip, more only lengthens the second stage -- but never fewer than 16 chunks where the rows allow them
constexpr int PLUMB_CS_ROWS = 512, PLUMB_CS_MAX_CHUNKS = 1024, PLUMB_CS_BLOCKS = 2048, PLUMB_CS_MIN_CHUNKS = 16;
// kd_bn_sums_finish: up to 256 partial rows go to the finishing kernel directly; more are staged, 64 rows a block up to 16384
// rows, 256 beyond
constexpr int PLUMB_BNS_DIRECT_ROWS = 256, PLUMB_BNS_LONG_ROWS = 16384, PLUMB_BNS_PER = 64, PLUMB_BNS_PER_LONG = 256;
// grid caps of the grid-stride kernels, tuned per file: broadcast_kernel (trunk_ops.hip), relu_bn_bwd / broadcast_add
// (bwd_ops.hip), the direct convolutions (small_ops.hip), copy_cast_kernel
constexpr int PLUMB_CAP_TRUNK = 8192, PLUMB_CAP_BWD = 16384, PLUMB_CAP_SMALL = 65536, PLUMB_CAP_COPY = 1 << 20;

struct PlumbGrid { unsigned x, y, z; };
struct PlumbSel {
    PlumbKernel kernel;
    PlumbGrid grid, grid2;      // the first and (two-launch entry points) the second pass
    int chunks, lc, cblocks;    // channel sums: row chunks, channel lanes of a block, channel blocks; bn sums: rows the finishing pass adds
    int per;                    // bn sums: rows per block of the staging pass (0: not staged)
    bool vec, flat4;            // 16-B accesses on every operand; upsample: four floats of the flattened (wo, c) row per thread
    float sh, sw, oh, ow;       // upsample: source coordinate = output coordinate * s + o
    bool two_pass;              // max-pool backward: arg-max bytes in the workspace, then the gather
    size_t ws_off[3];           // image pooling: byte offsets of the chunk partials, the means and the pooled vector in the workspace
    int blocks;                 // stem kernels: persistent workgroups
    int Ho, Wo, ngx, nseg;      // pooled extents; stem_pool: column groups and row segments per image; stem_conv (bf16): ngx = 16-column groups per row
};

// ---- predicates -----------------------------------------------------------------------------------------------------------------
static inline bool plumb_dtype_ok(int d) { return d == KD_F32 || d == KD_BF16; }
static inline int plumb_elem_size(int d) { return d == KD_BF16 ? 2 : 4; }
static inline bool plumb_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
// an absent operand, or one whose every pixel starts 16-B aligned
static inline bool plumb_vec_ok(const void *p, int ld, int es) { return !p || (plumb_aligned16(p) && (ld * es) % 16 == 0); }

// ---- grids ----------------------------------------------------------------------------------------------------------------------
// one thread per item, 256 a workgroup, at most `cap` workgroups (the kernels stride over the rest)
static inline unsigned plumb_grid(long long total, int cap)
{
    const long long b = (total + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}
static inline PlumbGrid plumb_grid3(long long x, long long y = 1, long long z = 1) { return PlumbGrid{(unsigned)x, (unsigned)y, (unsigned)z}; }
static inline PlumbSel plumb_flat(PlumbKernel k, long long blocks)
{
    PlumbSel c{};
    c.kernel = k;
    c.grid = c.grid2 = plumb_grid3(blocks);
    return c;
}
static inline int plumb_pool_out(int I) { return (I - 1) / 2 + 1; }     // 3x3 / stride 2 / pad 1

// the resampling geometry (resample.h) under the name the host wrapper of tests/plumb_select_host knows it by
typedef ResampleGeom PlumbUpGeom;
static inline PlumbUpGeom plumb_up_geom(int h, int w, int H, int W, int align_corners) { return resample_geom(h, w, H, W, align_corners); }

// ---- trunk_ops.hip --------------------------------------------------------------------------------------------------------------
static inline PlumbSel plumb_select_stem_conv(int dtype, int N, int H, int W)
{
    if (dtype != KD_BF16) return plumb_flat(PK_STEM_CONV_F32, ((long long)N * H * W + 63) / 64);     // 64 pixels a block
    const int gpr = (W + 15) / 16;
    const long long want = ((long long)N * H * gpr + 3) / 4;                                         // a 16-pixel group per wave and trip
    PlumbSel c = plumb_flat(PK_STEM_CONV_MFMA, want < PLUMB_STEM_MFMA_MAX_BLOCKS ? want : PLUMB_STEM_MFMA_MAX_BLOCKS);
    c.blocks = (int)c.grid.x;
    c.ngx = gpr;
    return c;
}
// PLUMB_REFUSED: more waves than four per block of a 2^31 - 1 block grid
static inline PlumbSel plumb_select_stem_conv_pool(int N, int H, int W)
{
    const int Ho = plumb_pool_out(H), Wo = plumb_pool_out(W);
    const int ngx = (Wo + PLUMB_SP_COLS - 1) / PLUMB_SP_COLS, nseg = (Ho + PLUMB_SP_ROWS - 1) / PLUMB_SP_ROWS;
    const long long waves = (long long)N * ngx * nseg;
    PlumbSel c = plumb_flat((waves + 3) / 4 <= 0x7fffffffLL ? PK_STEM_POOL : PLUMB_REFUSED, (waves + 3) / 4);
    c.Ho = Ho; c.Wo = Wo; c.ngx = ngx; c.nseg = nseg;
    return c;
}
// grid: x = chunks of one output row's (Wo * C/8) vectors, y = output row, z = image
static inline PlumbSel plumb_select_maxpool(int dtype, int N, int H, int W, int C)
{
    PlumbSel c{};
    c.kernel = (PlumbKernel)(PK_MAXPOOL_F32 + (dtype == KD_BF16));
    c.Ho = plumb_pool_out(H); c.Wo = plumb_pool_out(W);
    c.grid = c.grid2 = plumb_grid3(((long long)c.Wo * (C / 8) + 255) / 256, c.Ho, N);
    return c;
}
// flat4: dense fp32 rows of a channel count that is no multiple of 8 (the logits)
static inline PlumbSel plumb_select_upsample(const void *x, int x_dtype, int ldx, const void *y, int y_dtype, int ldy, int N, int H, int W, int C,
                                             int Ho, int Wo, int align_corners)
{
    PlumbSel c{};
    c.vec = C % 8 == 0 && plumb_vec_ok(x, ldx, plumb_elem_size(x_dtype)) && plumb_vec_ok(y, ldy, plumb_elem_size(y_dtype));
    c.flat4 = !c.vec && y_dtype == KD_F32 && ldy == C && ((long long)Wo * C) % 4 == 0 && plumb_aligned16(y);
    c.kernel = c.flat4 ? (PlumbKernel)(PK_UP_FLAT4_F32 + (x_dtype == KD_BF16))
                       : (PlumbKernel)(PK_UP_F32_F32_1 + 4 * (x_dtype == KD_BF16) + 2 * (y_dtype == KD_BF16) + c.vec);
    const long long per_row = c.flat4 ? (long long)Wo * C / 4 : (long long)Wo * (c.vec ? C / 8 : C);
    c.grid = c.grid2 = plumb_grid3((per_row + 255) / 256, (Ho + PLUMB_UP_RO - 1) / PLUMB_UP_RO, N);
    const ResampleGeom g = resample_geom(H, W, Ho, Wo, align_corners);
    c.sh = g.sh; c.sw = g.sw; c.oh = g.oh; c.ow = g.ow;
    return c;
}
// workspace: [chunk][n][c] partials | mean[n][c] | pooled vector [n][co], floats
static inline size_t plumb_image_pool_workspace(int N, int Cin, int Cout)
{
    return ((size_t)PLUMB_GAP_CHUNKS * N * Cin + (size_t)N * Cin + (size_t)N * Cout) * sizeof(float);
}
// grid: the chunk partials (kd_aspp_image_pool_sums: the row partials' finish, see below); grid2: the broadcast
static inline PlumbSel plumb_select_image_pool(int dtype, int N, int H, int W, int Cin, int Cout)
{
    PlumbSel c{};
    c.kernel = (PlumbKernel)(PK_GAP_PARTIAL_F32 + (dtype == KD_BF16));
    c.grid = plumb_grid3(PLUMB_GAP_CHUNKS, (Cin + 255) / 256, N);
    c.grid2 = plumb_grid3(plumb_grid((long long)N * H * W * (Cout / 8), PLUMB_CAP_TRUNK));
    c.ws_off[0] = 0;
    c.ws_off[1] = (size_t)PLUMB_GAP_CHUNKS * N * Cin * sizeof(float);
    c.ws_off[2] = c.ws_off[1] + (size_t)N * Cin * sizeof(float);
    return c;
}
// The pooled sums already taken by a conv epilogue: the same workspace and broadcast, gap_rows_finish_kernel (32 channels a block)
// in place of the two pooling launches.  `kernel` only carries the dtype of the broadcast: the entry point notes nothing.
static inline PlumbSel plumb_select_image_pool_sums(int dtype, int N, int H, int W, int Cin, int Cout)
{
    PlumbSel c = plumb_select_image_pool(dtype, N, H, W, Cin, Cout);
    c.grid = plumb_grid3((Cin + 31) / 32, N);
    return c;
}
static inline PlumbSel plumb_select_bn_fold(int C) { return plumb_flat(PK_BN_FOLD, (C + 255) / 256); }
static inline PlumbSel plumb_select_copy_cast(int64_t d_sC, int N, int C, int64_t P)
{
    return plumb_flat(d_sC == 1 ? PK_COPY_CAST_CFAST : PK_COPY_CAST_PFAST, plumb_grid((long long)N * C * P, PLUMB_CAP_COPY));
}

// ---- bwd_ops.hip ----------------------------------------------------------------------------------------------------------------
static inline PlumbSel plumb_select_relu_bn_bwd(int dtype, int64_t M, int C)
{
    return plumb_flat((PlumbKernel)(PK_RELU_BN_BWD_F32 + (dtype == KD_BF16)), plumb_grid((long long)M * (C / 8), PLUMB_CAP_BWD));
}
static inline int plumb_cs_chunks(long long rows)
{
    const long long c = (rows + PLUMB_CS_ROWS - 1) / PLUMB_CS_ROWS;
    return (int)(c < 1 ? 1 : (c > PLUMB_CS_MAX_CHUNKS ? PLUMB_CS_MAX_CHUNKS : c));
}
// part[group][chunk][2][C] floats, sized for the most chunks a call may take
static inline size_t plumb_channel_sums_workspace(int groups, int64_t rows, int C)
{
    return (size_t)groups * plumb_cs_chunks(rows) * 2 * (size_t)C * sizeof(float);
}
// grid: (row chunks, channel blocks of lc vectors, groups); grid2: the fp64 finish, 16 channels a block
static inline PlumbSel plumb_select_channel_sums(int dtype, const void *g, int ldg, const void *sub, int ldsub, const void *a, int lda, int groups,
                                                 int64_t rows, int C)
{
    const int es = plumb_elem_size(dtype);
    PlumbSel c{};
    c.vec = C % 8 == 0 && plumb_vec_ok(g, ldg, es) && plumb_vec_ok(sub, ldsub, es) && plumb_vec_ok(a, lda, es);
    c.kernel = (PlumbKernel)(PK_CS_F32_1 + 2 * (dtype == KD_BF16) + c.vec);
    const int nvec = c.vec ? (C + 7) / 8 : C;
    c.lc = nvec > 16 ? 32 : (nvec > 8 ? 16 : (nvec > 4 ? 8 : 4));   // channel lanes of a block, as in the kernel
    c.cblocks = (nvec + c.lc - 1) / c.lc;
    const int most = plumb_cs_chunks(rows);
    c.chunks = most;
    const long long other = (long long)groups * c.cblocks;
    const long long want = (PLUMB_CS_BLOCKS + other - 1) / (other > 0 ? other : 1);
    if (want < c.chunks) c.chunks = (int)(want < PLUMB_CS_MIN_CHUNKS ? PLUMB_CS_MIN_CHUNKS : want);
    if (c.chunks > most) c.chunks = most;       // never more than the workspace was sized for
    c.grid = plumb_grid3(c.chunks, c.cblocks, groups);
    c.grid2 = plumb_grid3((long long)groups * ((C + 15) / 16));
    return c;
}
static inline int plumb_bn_sums_per(int rows) { return rows > PLUMB_BNS_LONG_ROWS ? PLUMB_BNS_PER_LONG : PLUMB_BNS_PER; }
static inline int plumb_bn_sums_chunks(int rows) { return (int)(((long long)rows + plumb_bn_sums_per(rows) - 1) / plumb_bn_sums_per(rows)); }
static inline size_t plumb_bn_sums_finish_workspace(int rows, int C)
{
    return rows > PLUMB_BNS_DIRECT_ROWS ? (size_t)plumb_bn_sums_chunks(rows) * 2 * (size_t)C * sizeof(float) : 0;
}
// grid2: the finishing kernel over `chunks` rows; staged (per > 0): grid = (channel blocks of 16, chunks of `per` rows) first
static inline PlumbSel plumb_select_bn_sums_finish(int rows, int C)
{
    PlumbSel c = plumb_flat(PK_CS_FINISH, (C + 15) / 16);
    c.chunks = rows;
    if (rows > PLUMB_BNS_DIRECT_ROWS) {
        c.per = plumb_bn_sums_per(rows);
        c.chunks = plumb_bn_sums_chunks(rows);
        c.kernel = c.per == PLUMB_BNS_PER_LONG ? PK_BNS_STAGE_256 : PK_BNS_STAGE_64;
        c.grid.y = (unsigned)c.chunks;
    }
    return c;
}
static inline PlumbSel plumb_select_bn_eval_param_grads(int C) { return plumb_flat(PK_BN_EVAL_PARAM_GRADS, (C + 255) / 256); }
static inline size_t plumb_maxpool_bwd_workspace(int N, int H, int W, int C)
{
    return (size_t)N * ((H - 1) / 2 + 1) * ((W - 1) / 2 + 1) * (size_t)((C + 7) / 8) * 8;   // one byte per window and channel
}
// Without a workspace, with one too small or not 8-B aligned, the one-pass kernel (a selection, not a refusal).
// two_pass: grid = the arg-max over the windows, grid2 = the gather over the input pixels
static inline PlumbSel plumb_select_maxpool_bwd(int dtype, const void *x, int ldx, const void *gy, int ldgy, const void *gx, int ldgx, int N, int H,
                                                int W, int C, const void *workspace, size_t workspace_bytes)
{
    const int es = plumb_elem_size(dtype), bf = dtype == KD_BF16;
    PlumbSel c{};
    c.Ho = plumb_pool_out(H); c.Wo = plumb_pool_out(W);
    c.vec = C % 8 == 0 && plumb_vec_ok(x, ldx, es) && plumb_vec_ok(gy, ldgy, es) && plumb_vec_ok(gx, ldgx, es);
    c.two_pass = c.vec && workspace && workspace_bytes >= plumb_maxpool_bwd_workspace(N, H, W, C) && ((uintptr_t)workspace & 7) == 0;
    const long long cv = c.vec ? C / 8 : C;
    c.grid = c.grid2 = plumb_grid3((W * cv + 255) / 256, H, N);
    if (c.two_pass) c.grid = plumb_grid3((c.Wo * cv + 255) / 256, c.Ho, N);
    c.kernel = c.two_pass ? (PlumbKernel)(PK_MP_ARGMAX_F32 + bf) : (PlumbKernel)(PK_MPB_F32_1 + 2 * bf + c.vec);
    return c;
}
// tmp (N, Ho, W, C) floats between the pass along W and the pass along H
static inline size_t plumb_upsample_bwd_workspace(int N, int H, int W, int C, int Ho, int Wo)
{
    (void)H; (void)Wo;
    return (size_t)N * Ho * W * C * sizeof(float);
}
// gradient (N, Ho, Wo, C) -> (N, H, W, C): grid = the pass along W (Ho rows), grid2 = the pass along H; the forward's geometry
static inline PlumbSel plumb_select_upsample_bwd(const void *gy, int gy_dtype, int ldgy, const void *gx, int gx_dtype, int ldgx, int N, int H, int W,
                                                 int C, int Ho, int Wo, int align_corners, const void *workspace)
{
    PlumbSel c{};
    c.vec = C % 8 == 0 && plumb_vec_ok(gy, ldgy, plumb_elem_size(gy_dtype)) && plumb_vec_ok(gx, ldgx, plumb_elem_size(gx_dtype)) && plumb_aligned16(workspace);
    c.kernel = (PlumbKernel)(PK_UPB_F32_F32_1 + 4 * (gy_dtype == KD_BF16) + 2 * (gx_dtype == KD_BF16) + c.vec);
    const long long bx = ((long long)W * (c.vec ? C / 8 : C) + 255) / 256;
    c.grid = plumb_grid3(bx, Ho, N);
    c.grid2 = plumb_grid3(bx, H, N);
    const ResampleGeom g = resample_geom(H, W, Ho, Wo, align_corners);
    c.sh = g.sh; c.sw = g.sw; c.oh = g.oh; c.ow = g.ow;
    return c;
}
static inline PlumbSel plumb_select_zero_insert(int dtype, int N, int C, int Hy, int Wy)
{
    PlumbSel c{};
    c.kernel = (PlumbKernel)(PK_ZERO_INSERT_F32 + (dtype == KD_BF16));
    c.grid = c.grid2 = plumb_grid3(((long long)Wy * (C / 8) + 255) / 256, Hy, N);
    return c;
}
static inline PlumbSel plumb_select_broadcast_add(int dtype, int N, int64_t HW, int C)
{
    return plumb_flat((PlumbKernel)(PK_BCAST_ADD_F32 + (dtype == KD_BF16)), plumb_grid((long long)N * HW * (C / 8), PLUMB_CAP_BWD));
}
// persistent blocks over the (image row, PLUMB_SW_SEG-column segment) work items
static inline int plumb_stem_blocks(int N, int H, int W)
{
    const long long items = (long long)N * H * ((W + PLUMB_SW_SEG - 1) / PLUMB_SW_SEG);
    return (int)(items < PLUMB_STEM_MAX_BLOCKS ? items : PLUMB_STEM_MAX_BLOCKS);
}
static inline size_t plumb_stem_wgrad_workspace(int N, int H, int W) { return (size_t)plumb_stem_blocks(N, H, W) * 64 * 27 * sizeof(float); }
// The matrix-core kernel reads dy as 16-B pieces: bf16, ld_dy % 8 == 0, an aligned base.  grid2: the fixed-order finish.
static inline PlumbSel plumb_select_stem_wgrad(int dtype, const void *dy, int ld_dy, int N, int H, int W)
{
    const bool mfma = dtype == KD_BF16 && ld_dy % 8 == 0 && plumb_aligned16(dy);
    PlumbSel c = plumb_flat(mfma ? PK_STEM_WGRAD_MFMA : (PlumbKernel)(PK_STEM_WGRAD_F32 + (dtype == KD_BF16)), plumb_stem_blocks(N, H, W));
    c.blocks = (int)c.grid.x;
    c.grid2 = plumb_grid3((64 * 27 + 255) / 256);
    return c;
}

// ---- small_ops.hip --------------------------------------------------------------------------------------------------------------
// grid: one block per (output channel, input channel of its group) for dw; grid2: one per output channel for the bias gradient
static inline PlumbSel plumb_select_direct_wgrad(int K, int Cg)
{
    PlumbSel c = plumb_flat(PK_DCONV_WGRAD, (long long)K * Cg);
    c.grid2 = plumb_grid3(K);
    return c;
}
static inline PlumbSel plumb_select_bn2d_fwd(int training, int C) { return plumb_flat((PlumbKernel)(PK_BN2D_FWD_EVAL + (training != 0)), C); }   // a block per channel
static inline PlumbSel plumb_select_bn2d_bwd(int training, int C) { return plumb_flat((PlumbKernel)(PK_BN2D_BWD_EVAL + (training != 0)), C); }
