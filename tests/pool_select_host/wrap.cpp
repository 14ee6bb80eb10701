// C entry points over csrc/pool_select.h for tests/test_pool_select_host.py (ctypes) and sweep_main.cpp: the selectors with their
// pointers flattened to their 64-bit values and their result flattened to doubles, the predicates, the constants and the name the
// launchers note for each kernel value.
#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/pool_select.h"

namespace {
const void *ptr(long long v) { return (const void *)(uintptr_t)v; }
void flatten(const PoolSel &s, double *out)
{
    const double v[11] = {(double)s.kernel,   (double)s.vec,    (double)s.windows,     (double)s.cells,          (double)s.grid, (double)s.nwb,
                          (double)s.part_x,   (double)s.part_y, (double)s.finish,      (double)s.sums_offset,    (double)s.workspace_bytes};
    for (int i = 0; i < 11; ++i) out[i] = v[i];
}
}  // namespace

extern "C" {
const char *ps_name(int k) { return pool_kernel_name(k); }
int ps_count(void) { return POOL_COUNT; }
long long ps_const(int i)
{
    const long long v[] = {POOL_TPB, POOL_VEC, POOL_VEC_BYTES, POOL_CBLOCK, POOL_WINS, POOL_FINISH_CH, POOL_CAP, PK_FWD_1, PK_FWD_V, PK_BWD_1, PK_BWD_V};
    return i >= 0 && i < (int)(sizeof(v) / sizeof(v[0])) ? v[i] : -1;
}
int ps_shape_ok(int N, int H, int W, int C, int ldx, int ldo) { return pool_shape_ok(N, H, W, C, ldx, ldo); }
int ps_vec_ok(int C, long long a, int lda, long long b, int ldb, long long c, int ldc)
{
    return pool_vec_ok(C, ptr(a), lda, ptr(b), ldb, ptr(c), ldc);
}
double ps_workspace(int N, int H, int W, int C) { return (double)pool_workspace(N, H, W, C); }
// out: kernel, vec, windows, cells, grid, nwb, part_x, part_y, finish, sums_offset, workspace_bytes
void ps_select_fwd(int N, int H, int W, int C, long long x, int ldx, long long y, int ldy, double *out)
{
    flatten(pool_select_fwd(N, H, W, C, ptr(x), ldx, ptr(y), ldy), out);
}
void ps_select_bwd(int bn, int N, int H, int W, int C, long long x, int ldx, long long g, int ldg, long long dx, int lddx, double *out)
{
    flatten(pool_select_bwd(bn != 0, N, H, W, C, ptr(x), ldx, ptr(g), ldg, ptr(dx), lddx), out);
}
}
