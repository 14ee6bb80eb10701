// C entry points over csrc/bn_lp_select.h for tests/test_bn_lp_select_host.py (ctypes) and sweep_main.cpp: both selectors with
// their operands flattened -- a pointer is its 64-bit value, 0 an absent operand -- their result flattened to doubles, the
// constants, the grid helper, the view predicate, the workspace size and the name the launchers note for each kernel value.
#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/bn_lp_select.h"

namespace {
const void *ptr(long long v) { return (const void *)(uintptr_t)v; }
// out: kernel, vec, nrb, part_x, part_y, finish, grid
void flat(const BnLpSel &c, double *out)
{
    const double v[7] = {(double)c.kernel, (double)c.vec, (double)c.nrb, (double)c.part_x, (double)c.part_y, (double)c.finish, (double)c.grid};
    for (int i = 0; i < 7; ++i) out[i] = v[i];
}
}  // namespace

extern "C" {
const char *bl_name(int k) { return bn_lp_kernel_name(k); }
int bl_count(void) { return BN_LP_COUNT; }
long long bl_const(int i)
{
    const long long v[] = {BN_LP_ROWS, BN_LP_TPB, BN_LP_CBLOCK, BN_LP_VEC, BN_LP_CAP, BN_LP_FWD_FINISH_CH, BN_LP_BWD_FINISH_CH};
    return i >= 0 && i < (int)(sizeof(v) / sizeof(v[0])) ? v[i] : -1;
}
unsigned bl_grid(long long total) { return bn_lp_grid(total); }
int bl_view_ok(long long p, int ld) { return bn_lp_view_ok(ptr(p), ld); }
unsigned long long bl_workspace(long long M, int C) { return bn_lp_workspace(M, C); }
unsigned long long bl_sums_offset(long long M, int C) { return bn_lp_sums_offset(M, C); }
void bl_fwd(long long x, int ldx, long long y, int ldy, long long M, int C, double *out) { flat(bn_lp_select_fwd(ptr(x), ldx, ptr(y), ldy, M, C), out); }
void bl_bwd(long long gy, int ldg, long long x, int ldx, long long y, int ldy, long long res, int ldres, long long dx, int lddx, long long M, int C,
            double *out)
{
    flat(bn_lp_select_bwd(ptr(gy), ldg, ptr(x), ldx, ptr(y), ldy, ptr(res), ldres, ptr(dx), lddx, M, C), out);
}
}
