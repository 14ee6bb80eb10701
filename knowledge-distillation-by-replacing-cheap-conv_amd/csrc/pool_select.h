// Which kernels the fused BatchNorm -> ReLU -> MaxPool2d(2, 2) entry points (pool_ops.hip: kd_bn_relu_maxpool2x2_fwd / _bwd) run
// for a call, on what grids, and how many bytes of the caller's workspace the backward's partial sums take: a pure function of the
// shape, the pixel strides and the pointer values of the activation operands.  The launchers check their arguments, call
// pool_select_fwd() / pool_select_bwd(), note pool_kernel_name(sel.kernel) and launch what sel says.  No HIP, no getenv and no
// globals here: a plain host C++ compiler accepts this file, and tests/test_pool_select_host.py holds it to both sides of every gate.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/kdcc.h"

// One value per name the launchers note: pass (forward, backward) x accesses (scalar, 16 B), then POOL_COUNT.
enum PoolKernel { PK_FWD_1, PK_FWD_V, PK_BWD_1, PK_BWD_V, POOL_COUNT };
static inline const char *pool_kernel_name(int k)
{
    static const char *const names[] = {"pool_fwd_kernel<1>", "pool_fwd_kernel<4>", "pool_bwd_kernel<1>", "pool_bwd_kernel<4>"};
    static_assert(sizeof(names) / sizeof(names[0]) == POOL_COUNT, "one name per kernel value");
    return k >= 0 && k < POOL_COUNT ? names[k] : nullptr;
}

// What pool_ops.hip is built for; it aliases these or static_asserts against them.
constexpr int POOL_TPB = 256;         // threads of every workgroup
constexpr int POOL_VEC = 4;           // channels of one 16-B access
constexpr int POOL_VEC_BYTES = 16;
constexpr int POOL_CBLOCK = 64;       // channels of a stage-1 workgroup: 64 lanes x 1 channel or 16 lanes x 4 channels
constexpr int POOL_WINS = 48;         // 2x2 windows of a stage-1 workgroup: 3 per thread at 16-B accesses, 12 at scalar ones; 192 pixels, so
                                      // a pass has no more window blocks than a BatchNorm pass over the same pixels has row blocks (128)
constexpr int POOL_FINISH_CH = 64;    // channels per workgroup of the fp64 stage 2 (bn_nhwc_core.h's bn_nhwc_grad_finish_kernel)
constexpr int POOL_CAP = 8192;        // workgroups of the grid-stride passes at most

struct PoolSel {
    PoolKernel kernel;
    int vec;                    // channels a thread loads (and stores) at once: 1 or 4
    long long windows;          // N * (H / 2) * (W / 2): the pooled pixels, one 2x2 window each
    long long cells;            // N * ceil(H / 2) * ceil(W / 2): the windows plus the partial ones of a dropped odd row / column
    unsigned grid;              // the grid-stride pass: the forward over windows, the backward's dx pass over cells, x C / vec
    int nwb;                    // stage 1 of the backward: window blocks = ceil(windows / POOL_WINS) ...
    unsigned part_x, part_y;    // ... its grid (window blocks, channel blocks of POOL_CBLOCK) ...
    unsigned finish;            // ... and stage 2's: channel blocks of POOL_FINISH_CH
    size_t sums_offset;         // floats: part[window block][2][C] | sums[2][C]
    size_t workspace_bytes;     // what the backward needs of the caller's workspace (0: the forward, the no-BN form)
};

// ---- predicates -----------------------------------------------------------------------------------------------------------------
static inline bool pool_aligned16(const void *p) { return ((uintptr_t)p & (POOL_VEC_BYTES - 1)) == 0; }
// N, C >= 1, a map that holds one window, pixel strides that hold the channels (ldo: the second view's, 0 when it is absent)
static inline bool pool_shape_ok(int32_t N, int32_t H, int32_t W, int32_t C, int32_t ldx, int32_t ldo)
{
    return N >= 1 && H >= 2 && W >= 2 && C >= 1 && ldx >= C && (ldo == 0 || ldo >= C);
}
// an absent view, or one whose every pixel starts 16-B aligned
static inline bool pool_view_ok(const void *p, int32_t ld) { return p == nullptr || (pool_aligned16(p) && ld % POOL_VEC == 0); }
// 16-B accesses need whole channel groups and every view of the call to allow them; a NULL view puts no condition on its stride
static inline bool pool_vec_ok(int32_t C, const void *a, int32_t lda, const void *b, int32_t ldb, const void *c, int32_t ldc)
{
    return C % POOL_VEC == 0 && pool_view_ok(a, lda) && pool_view_ok(b, ldb) && pool_view_ok(c, ldc);
}

// ---- grids and the workspace ------------------------------------------------------------------------------------------------------
static inline unsigned pool_grid(long long items)
{
    const long long b = (items + POOL_TPB - 1) / POOL_TPB;
    return (unsigned)(b < 1 ? 1 : (b > POOL_CAP ? POOL_CAP : b));
}
static inline long long pool_windows(int32_t N, int32_t H, int32_t W) { return (long long)N * (H / 2) * (W / 2); }
static inline long long pool_cells(int32_t N, int32_t H, int32_t W) { return (long long)N * ((H + 1) / 2) * ((W + 1) / 2); }
static inline int pool_window_blocks(long long windows) { return (int)((windows + POOL_WINS - 1) / POOL_WINS); }
// bytes of the backward's partials and sums: never more than kd_bn_nhwc_workspace(N H W, C), which the caller provides
static inline size_t pool_workspace(int32_t N, int32_t H, int32_t W, int32_t C)
{
    if (N <= 0 || H < 2 || W < 2 || C <= 0) return 0;
    return ((size_t)pool_window_blocks(pool_windows(N, H, W)) * 2 * (size_t)C + 2 * (size_t)C) * sizeof(float);
}

// ---- the entry points -----------------------------------------------------------------------------------------------------------
static inline PoolSel pool_plan(bool backward, bool vec, bool sums, int32_t N, int32_t H, int32_t W, int32_t C)
{
    PoolSel s{};
    s.vec = vec ? POOL_VEC : 1;
    s.kernel = (PoolKernel)((backward ? 2 : 0) + (vec ? 1 : 0));
    s.windows = pool_windows(N, H, W);
    s.cells = pool_cells(N, H, W);
    s.grid = pool_grid((backward ? s.cells : s.windows) * (C / s.vec));
    if (backward && sums) {
        s.nwb = pool_window_blocks(s.windows);
        s.part_x = (unsigned)s.nwb;
        s.part_y = (unsigned)((C + POOL_CBLOCK - 1) / POOL_CBLOCK);
        s.finish = (unsigned)((C + POOL_FINISH_CH - 1) / POOL_FINISH_CH);
        s.sums_offset = (size_t)s.nwb * 2 * (size_t)C;
        s.workspace_bytes = pool_workspace(N, H, W, C);
    }
    return s;
}
static inline PoolSel pool_select_fwd(int32_t N, int32_t H, int32_t W, int32_t C, const void *x, int32_t ldx, const void *y, int32_t ldy)
{
    return pool_plan(false, pool_vec_ok(C, x, ldx, y, ldy, nullptr, 0), false, N, H, W, C);
}
// bn: the call has BatchNorm operands (gamma given), so the two reduction stages run; dx may be NULL
static inline PoolSel pool_select_bwd(bool bn, int32_t N, int32_t H, int32_t W, int32_t C, const void *x, int32_t ldx, const void *g, int32_t ldg,
                                      const void *dx, int32_t lddx)
{
    return pool_plan(true, pool_vec_ok(C, x, ldx, g, ldg, dx, lddx), bn, N, H, W, C);
}
