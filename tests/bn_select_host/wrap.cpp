// C entry points over csrc/bn_select.h for tests/test_bn_select_host.py, tests/test_nhwc_support_host.py (ctypes) and
// sweep_main.cpp: both selectors with their operands flattened -- a pointer is its 64-bit value, 0 an absent operand -- their
// result flattened to doubles, the constants, the grid helper, the predicates, the workspace size and the name the launchers
// note for each kernel value.  es is the element size: 4 (fp32) or 2 (bf16).
#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/bn_select.h"

namespace {
const void *ptr(long long v) { return (const void *)(uintptr_t)v; }
// out: kernel, vec, part_vec, nrb, part_x, part_y, finish, grid
void flat(const BnSel &c, double *out)
{
    const double v[8] = {(double)c.kernel, (double)c.vec, (double)c.part_vec, (double)c.nrb, (double)c.part_x, (double)c.part_y, (double)c.finish,
                         (double)c.grid};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
}
}  // namespace

extern "C" {
const char *bl_name(int k) { return bn_kernel_name(k); }
int bl_count(void) { return BN_KERNEL_COUNT; }
long long bl_const(int i)
{
    const long long v[] = {BN_ROWS, BN_TPB, BN_CBLOCK, BN_VEC_BYTES, BN_CAP, BN_FWD_FINISH_CH, BN_BWD_FINISH_CH};
    return i >= 0 && i < (int)(sizeof(v) / sizeof(v[0])) ? v[i] : -1;
}
unsigned bl_grid(long long total) { return bn_grid(total); }
int bl_view_ok(int es, long long p, int ld) { return bn_view_ok(es, ptr(p), ld); }
int bl_vec_ok(int es, int C, long long a, int lda, long long b, int ldb) { return bn_vec_ok(es, C, ptr(a), lda, ptr(b), ldb); }
unsigned long long bl_workspace(long long M, int C) { return bn_workspace(M, C); }
unsigned long long bl_sums_offset(long long M, int C) { return bn_sums_offset(M, C); }
void bl_fwd(int es, long long x, int ldx, long long y, int ldy, long long M, int C, double *out)
{
    flat(bn_select_fwd(es, ptr(x), ldx, ptr(y), ldy, M, C), out);
}
void bl_bwd(int es, long long gy, int ldg, long long x, int ldx, long long y, int ldy, long long res, int ldres, long long dx, int lddx, long long M,
            int C, double *out)
{
    flat(bn_select_bwd(es, ptr(gy), ldg, ptr(x), ldx, ptr(y), ldy, ptr(res), ldres, ptr(dx), lddx, M, C), out);
}
}
