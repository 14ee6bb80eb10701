// C entry points over csrc/dropout_rng.h and csrc/dropout_select.h for tests/test_dropout_host.py (ctypes) and sweep_main.cpp: the
// generator, the keep decision (one index, or an array of them), the value rule, and the selector with its pointers flattened to
// their 64-bit values and its result flattened to doubles, the predicates, the constants and the name the launcher notes.
#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/dropout_rng.h"
#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/dropout_select.h"

namespace {
const void *ptr(long long v) { return (const void *)(uintptr_t)v; }
}  // namespace

extern "C" {
// ---- dropout_rng.h
void dr_philox(const uint32_t *ctr, const uint32_t *key, uint32_t *out)
{
    const PhiloxBlock b = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    for (int i = 0; i < 4; ++i) out[i] = b.w[i];
}
long long dr_const(int i)
{
    const long long v[] = {PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1, PHILOX_ROUNDS, DROPOUT_WORDS};
    return i >= 0 && i < (int)(sizeof(v) / sizeof(v[0])) ? v[i] : -1;
}
int dr_keep(uint64_t seed, uint64_t offset, int64_t idx, uint32_t threshold) { return dropout_keep(seed, offset, idx, threshold); }
void dr_keep_many(uint64_t seed, uint64_t offset, const int64_t *idx, int64_t n, uint32_t threshold, uint8_t *out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = dropout_keep(seed, offset, idx[i], threshold);
}
float dr_apply(float x, int keep, float scale) { return dropout_apply(x, keep != 0, scale); }

// ---- dropout_select.h
const char *ds_name(int k) { return dropout_kernel_name(k); }
int ds_count(void) { return DROPOUT_COUNT; }
long long ds_const(int i)
{
    const long long v[] = {DROPOUT_TPB, DROPOUT_CAP, DROPOUT_VEC_BYTES, DROPOUT_BLOCK, DK_F32_1, DK_F32_V, DK_BF16_1, DK_BF16_V};
    return i >= 0 && i < (int)(sizeof(v) / sizeof(v[0])) ? v[i] : -1;
}
int ds_args_ok(long long x, int ldx, long long y, int ldy, int dtype, long long M, int C)
{
    return dropout_args_ok(ptr(x), ldx, ptr(y), ldy, dtype, M, C);
}
int ds_vec_ok(int dtype, int C, long long x, int ldx, long long y, int ldy) { return dropout_vec_ok(dtype, C, ptr(x), ldx, ptr(y), ldy); }
long long ds_grid(long long items) { return dropout_grid(items); }
// out: kernel, vec, items, grid
void ds_select(int dtype, long long M, int C, long long x, int ldx, long long y, int ldy, double *out)
{
    const DropoutSel s = dropout_select(dtype, M, C, ptr(x), ldx, ptr(y), ldy);
    const double v[4] = {(double)s.kernel, (double)s.vec, (double)s.items, (double)s.grid};
    for (int i = 0; i < 4; ++i) out[i] = v[i];
}
}
