// Which kernels the bf16 NHWC BatchNorm entry points (bn_nhwc_lp.hip: kd_bn_nhwc_lp_fwd / _bwd) run for a call, and on what grids:
// a pure function of the shape and of the operands' pointer values and leading dimensions.  The launchers check their arguments,
// call the selector of their entry point, note bn_lp_kernel_name(sel.kernel) and launch what sel says; kd_bn_nhwc_lp_workspace
// returns bn_lp_workspace().  No HIP, no getenv and no globals here: a plain host C++ compiler accepts this file, and
// tests/test_bn_lp_select_host.py holds it to both sides of every gate.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/kdcc.h"

// One value per name the launchers note, scalar before vector (kernel + vec), then BN_LP_COUNT.
enum BnLpKernel {
    BLP_APPLY_1, BLP_APPLY_8,   // forward: the normalise (+ ReLU) pass; the statistics partials before it take the same variant
    BLP_DX_1, BLP_DX_8,         // backward with dx: the input-gradient pass (the reduction partials take the same variant)
    BLP_GRAD_1, BLP_GRAD_8,     // backward without dx: the reduction alone (parameter gradients only)
    BN_LP_COUNT,
};
static inline const char *bn_lp_kernel_name(int k)
{
    static const char *const names[] = {"bn_lp_apply_kernel<1>", "bn_lp_apply_kernel<8>", "bn_lp_dx_kernel<1>", "bn_lp_dx_kernel<8>",
                                        "bn_lp_grad_partial_kernel<1>", "bn_lp_grad_partial_kernel<8>"};
    static_assert(sizeof(names) / sizeof(names[0]) == BN_LP_COUNT, "one name per kernel value");
    return k >= 0 && k < BN_LP_COUNT ? names[k] : nullptr;
}
static_assert(BLP_APPLY_8 == BLP_APPLY_1 + 1 && BLP_DX_8 == BLP_DX_1 + 1 && BLP_GRAD_8 == BLP_GRAD_1 + 1,
              "the selectors compute the vector variant from the order of BnLpKernel");

// What bn_nhwc_lp.hip is built for; it aliases these or static_asserts against them (and against bn_nhwc_core.h's).
constexpr int BN_LP_ROWS = 128;         // pixels per stage-1 workgroup: the fp32 kernels' blocking, so the stage-2 finish is shared
constexpr int BN_LP_TPB = 256;          // threads of every workgroup
constexpr int BN_LP_CBLOCK = 64;        // channels of a stage-1 workgroup: 64 lanes x 1 channel or 8 lanes x 8 channels
constexpr int BN_LP_VEC = 8;            // channels a lane of the vector kernels owns: 16 B of bf16
constexpr int BN_LP_CAP = 8192;         // workgroups of the grid-stride passes at most, as the fp32 kernels
constexpr int BN_LP_FWD_FINISH_CH = 16; // channels per workgroup of the forward's fp64 finish (bn_nhwc_stats_finish_kernel)
constexpr int BN_LP_BWD_FINISH_CH = 64; // channels per workgroup of the backward's fp64 finish

struct BnLpSel {
    BnLpKernel kernel;
    bool vec;                   // 16-B accesses, 8 channels a lane, on every operand of the call
    int nrb;                    // stage-1 row blocks = ceil(M / BN_LP_ROWS)
    unsigned part_x, part_y;    // stage 1: (row blocks, channel blocks of BN_LP_CBLOCK)
    unsigned finish;            // stage 2: channel blocks of the fp64 finish
    unsigned grid;              // the grid-stride elementwise pass (apply / dx)
};

// ---- predicates -----------------------------------------------------------------------------------------------------------------
static inline bool bn_lp_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
// an absent operand, or a bf16 view whose every pixel starts 16-B aligned (ld in elements)
static inline bool bn_lp_view_ok(const void *p, int ld) { return !p || (bn_lp_aligned16(p) && ((long long)ld * 2) % 16 == 0); }

// ---- grids and the workspace ------------------------------------------------------------------------------------------------------
// one thread per item, BN_LP_TPB a workgroup, at most BN_LP_CAP workgroups (the kernels stride over the rest)
static inline unsigned bn_lp_grid(long long total)
{
    const long long b = (total + BN_LP_TPB - 1) / BN_LP_TPB;
    return (unsigned)(b < 1 ? 1 : (b > BN_LP_CAP ? BN_LP_CAP : b));
}
static inline int bn_lp_row_blocks(int64_t M) { return (int)((M + BN_LP_ROWS - 1) / BN_LP_ROWS); }
// floats: part[row block][3][C] (the forward's k / sum / sum of squares; the backward uses [row block][2][C] of it) | sums[2][C]
static inline size_t bn_lp_workspace(int64_t M, int32_t C)
{
    if (M <= 0 || C <= 0) return 0;
    return ((size_t)bn_lp_row_blocks(M) * 3 * (size_t)C + 2 * (size_t)C) * sizeof(float);
}
// float offset of sums[2][C] behind the partials
static inline size_t bn_lp_sums_offset(int64_t M, int32_t C) { return (size_t)bn_lp_row_blocks(M) * 3 * (size_t)C; }

static inline BnLpSel bn_lp_plan(BnLpKernel scalar, bool vec, int64_t M, int32_t C, int finish_ch)
{
    BnLpSel s{};
    s.vec = vec;
    s.kernel = (BnLpKernel)(scalar + vec);
    s.nrb = bn_lp_row_blocks(M);
    s.part_x = (unsigned)s.nrb;
    s.part_y = (unsigned)((C + BN_LP_CBLOCK - 1) / BN_LP_CBLOCK);
    s.finish = (unsigned)((C + finish_ch - 1) / finish_ch);
    s.grid = bn_lp_grid((long long)M * (vec ? C / BN_LP_VEC : C));
    return s;
}

// ---- the entry points ---------------------------------------------------------------------------------------------------------------
static inline BnLpSel bn_lp_select_fwd(const void *x, int ldx, const void *y, int ldy, int64_t M, int32_t C)
{
    const bool vec = C % BN_LP_VEC == 0 && bn_lp_view_ok(x, ldx) && bn_lp_view_ok(y, ldy);
    return bn_lp_plan(BLP_APPLY_1, vec, M, C, BN_LP_FWD_FINISH_CH);
}
// y is the operand the call reads: NULL without relu; res and dx may be absent
static inline BnLpSel bn_lp_select_bwd(const void *gy, int ldg, const void *x, int ldx, const void *y, int ldy, const void *res, int ldres,
                                       const void *dx, int lddx, int64_t M, int32_t C)
{
    const bool vec = C % BN_LP_VEC == 0 && bn_lp_view_ok(gy, ldg) && bn_lp_view_ok(x, ldx) && bn_lp_view_ok(y, ldy) && bn_lp_view_ok(res, ldres) &&
                     bn_lp_view_ok(dx, lddx);
    return bn_lp_plan(dx ? BLP_DX_1 : BLP_GRAD_1, vec, M, C, BN_LP_BWD_FINISH_CH);
}
