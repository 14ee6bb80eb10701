// Which kernels the NHWC BatchNorm entry points run for a call, and on what grids: bn_nhwc.hip's kd_bn_nhwc_fwd / _bwd (fp32,
// es = 4) and kd_bn_nhwc_lp_fwd / _bwd (bf16, es = 2), dense_ops.hip's kd_bn_nhwc_stats / _apply.  A pure function of the element
// size, the shape and the operands' pointer values and leading dimensions.  The implementations in bn_nhwc_core.h check their
// arguments, call the selector of their entry point, note bn_kernel_name(sel.kernel) and launch what sel says; the workspace
// entry points return bn_workspace().  dense_ops.hip's average-pool launchers take their float4 gate and grid from bn_view_ok /
// bn_grid.  No HIP, no getenv and no globals here: a plain host C++ compiler accepts this file, and tests/test_bn_select_host.py
// holds it to both sides of every gate.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/kdcc.h"

// One value per name the launchers note, scalar before vector, fp32 before bf16, then BN_KERNEL_COUNT.
enum BnKernel {
    BN_F32_APPLY_1, BN_F32_APPLY_4,     // forward: the normalise (+ ReLU) pass
    BN_F32_DX_1, BN_F32_DX_4,           // backward with dx: the input-gradient pass
    BN_F32_GRAD_1,                      // backward without dx: the reduction alone; the fp32 partials are always scalar
    BN_BF16_APPLY_1, BN_BF16_APPLY_8,   // the bf16 partials take the variant of the elementwise pass
    BN_BF16_DX_1, BN_BF16_DX_8,
    BN_BF16_GRAD_1, BN_BF16_GRAD_8,
    BN_KERNEL_COUNT,
};
// The names are what last_plumbing_kernel() answered before the two storages shared one implementation, and what the tests and
// profiles/ know: labels of the choice (storage, kind, width), not the templates' symbols.  bn_nhwc_* is the fp32 storage and
// bn_lp_* the bf16 one; the fp32 backward without dx is noted by its finish kernel.
static inline const char *bn_kernel_name(int k)
{
    static const char *const names[] = {
        "bn_nhwc_apply_kernel<1>", "bn_nhwc_apply_kernel<4>", "bn_nhwc_dx_kernel<1>", "bn_nhwc_dx_kernel<4>",
        "bn_nhwc_grad_finish_kernel",
        "bn_lp_apply_kernel<1>", "bn_lp_apply_kernel<8>", "bn_lp_dx_kernel<1>", "bn_lp_dx_kernel<8>",
        "bn_lp_grad_partial_kernel<1>", "bn_lp_grad_partial_kernel<8>"};
    static_assert(sizeof(names) / sizeof(names[0]) == BN_KERNEL_COUNT, "one name per kernel value");
    return k >= 0 && k < BN_KERNEL_COUNT ? names[k] : nullptr;
}
static_assert(BN_F32_APPLY_4 == BN_F32_APPLY_1 + 1 && BN_F32_DX_4 == BN_F32_DX_1 + 1 && BN_BF16_APPLY_8 == BN_BF16_APPLY_1 + 1 &&
                  BN_BF16_DX_8 == BN_BF16_DX_1 + 1 && BN_BF16_GRAD_8 == BN_BF16_GRAD_1 + 1,
              "the selectors compute the vector variant from the order of BnKernel");

// What bn_nhwc_core.h is built for; it static_asserts against these.
constexpr int BN_ROWS = 128;            // pixels per stage-1 workgroup
constexpr int BN_TPB = 256;             // threads of every workgroup
constexpr int BN_CBLOCK = 64;           // channels of a stage-1 workgroup: 64 lanes x 1 channel or (bf16) 8 lanes x 8 channels
constexpr int BN_VEC_BYTES = 16;        // bytes a lane of the vector kernels owns: 4 fp32 or 8 bf16 channels
constexpr int BN_CAP = 8192;            // workgroups of the grid-stride passes at most
constexpr int BN_FWD_FINISH_CH = 16;    // channels per workgroup of the forward's fp64 finish (bn_nhwc_stats_finish_kernel)
constexpr int BN_BWD_FINISH_CH = 64;    // channels per workgroup of the backward's fp64 finish (bn_nhwc_grad_finish_kernel)

struct BnSel {
    BnKernel kernel;
    bool vec;                   // the elementwise pass takes 16 B a lane (V = 16 / es channels) on every operand of the call
    bool part_vec;              // the stage-1 partials take the vector variant: bf16 only (4-channel fp32 partials would sum in another order)
    int nrb;                    // stage-1 row blocks = ceil(M / BN_ROWS)
    unsigned part_x, part_y;    // stage 1: (row blocks, channel blocks of BN_CBLOCK)
    unsigned finish;            // stage 2: channel blocks of the fp64 finish
    unsigned grid;              // the grid-stride elementwise pass (apply / dx)
};

// ---- predicates -----------------------------------------------------------------------------------------------------------------
static inline bool bn_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
// an absent operand, or a view of es-byte elements whose every pixel starts 16-B aligned (ld in elements)
static inline bool bn_view_ok(int es, const void *p, int ld) { return !p || (bn_aligned16(p) && ((long long)ld * es) % BN_VEC_BYTES == 0); }
static inline bool bn_channels_ok(int es, int32_t C) { return C % (BN_VEC_BYTES / es) == 0; }
// the 16-B gate of a pass over two views (the forward's x -> y; with es = 4 the average pools' float4 gate)
static inline bool bn_vec_ok(int es, int32_t C, const void *a, int lda, const void *b, int ldb)
{
    return bn_channels_ok(es, C) && bn_view_ok(es, a, lda) && bn_view_ok(es, b, ldb);
}

// ---- grids and the workspace ------------------------------------------------------------------------------------------------------
// one thread per item, BN_TPB a workgroup, at most BN_CAP workgroups (the kernels stride over the rest)
static inline unsigned bn_grid(long long total)
{
    const long long b = (total + BN_TPB - 1) / BN_TPB;
    return (unsigned)(b < 1 ? 1 : (b > BN_CAP ? BN_CAP : b));
}
static inline int bn_row_blocks(int64_t M) { return (int)((M + BN_ROWS - 1) / BN_ROWS); }
// floats, whatever the storage: part[row block][3][C] (the forward's k / sum / sum of squares; the backward uses
// [row block][2][C] of it) | sums[2][C]
static inline size_t bn_workspace(int64_t M, int32_t C)
{
    if (M <= 0 || C <= 0) return 0;
    return ((size_t)bn_row_blocks(M) * 3 * (size_t)C + 2 * (size_t)C) * sizeof(float);
}
// float offset of sums[2][C] behind the partials
static inline size_t bn_sums_offset(int64_t M, int32_t C) { return (size_t)bn_row_blocks(M) * 3 * (size_t)C; }

// scalar: the scalar kernel of the call's kind and storage; by_part: the noted kernel is a stage-1 partial (no elementwise pass runs)
static inline BnSel bn_plan(int es, BnKernel scalar, bool by_part, bool vec, int64_t M, int32_t C, int finish_ch)
{
    BnSel s{};
    s.vec = vec;
    s.part_vec = vec && es == 2;
    s.kernel = (BnKernel)(scalar + (by_part ? s.part_vec : vec));
    s.nrb = bn_row_blocks(M);
    s.part_x = (unsigned)s.nrb;
    s.part_y = (unsigned)((C + BN_CBLOCK - 1) / BN_CBLOCK);
    s.finish = (unsigned)((C + finish_ch - 1) / finish_ch);
    s.grid = bn_grid((long long)M * (vec ? C / (BN_VEC_BYTES / es) : C));
    return s;
}

// ---- the entry points ---------------------------------------------------------------------------------------------------------------
// es: 4 (fp32) or 2 (bf16).  kd_bn_nhwc_apply (no statistics of its own) takes the forward's answer and launches its elementwise part.
static inline BnSel bn_select_fwd(int es, const void *x, int ldx, const void *y, int ldy, int64_t M, int32_t C)
{
    return bn_plan(es, es == 2 ? BN_BF16_APPLY_1 : BN_F32_APPLY_1, false, bn_vec_ok(es, C, x, ldx, y, ldy), M, C, BN_FWD_FINISH_CH);
}
// y is the operand the call reads: NULL without relu; res and dx may be absent
static inline BnSel bn_select_bwd(int es, const void *gy, int ldg, const void *x, int ldx, const void *y, int ldy, const void *res, int ldres,
                                  const void *dx, int lddx, int64_t M, int32_t C)
{
    const bool vec = bn_vec_ok(es, C, gy, ldg, x, ldx) && bn_view_ok(es, y, ldy) && bn_view_ok(es, res, ldres) && bn_view_ok(es, dx, lddx);
    const BnKernel scalar = es == 2 ? (dx ? BN_BF16_DX_1 : BN_BF16_GRAD_1) : (dx ? BN_F32_DX_1 : BN_F32_GRAD_1);
    return bn_plan(es, scalar, !dx, vec, M, C, BN_BWD_FINISH_CH);
}
