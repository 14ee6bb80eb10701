// C entry points over csrc/seg_stats_select.h for tests/test_cityscapes_uniform_host.py (ctypes) and sweep_main.cpp: the selector
// with its pointer flattened to a 64-bit value and its result flattened to doubles, the rows-per-workgroup rule for any byte budget,
// the class-count predicate, the constants and the name the launcher notes for each kernel value.
#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/seg_stats_select.h"

extern "C" {
const char *st_name(int k) { return seg_stats_kernel_name(k); }
int st_count(void) { return SEG_STATS_COUNT; }
long long st_const(int i)
{
    const long long v[] = {SEG_STATS_TPB, SEG_STATS_MAX_CLASSES, SEG_STATS_WG_BYTES, SEG_STATS_MAX_GRID, SEG_MAX_SIDE, SSK_STATS_1, SSK_STATS_16};
    return i >= 0 && i < (int)(sizeof(v) / sizeof(v[0])) ? v[i] : -1;
}
int st_classes_ok(int c) { return seg_stats_classes_ok(c); }
int st_rows(int tile, long long budget) { return seg_stats_rows(tile, budget); }
// out: kernel, launch, vec, th, tw, rows, chunks, units, grid
void st_select(long long targets, long long n, int H, int W, int tile, double *out)
{
    const SegStatsSel s = seg_stats_select((const void *)(uintptr_t)targets, n, H, W, tile);
    const double v[9] = {(double)s.kernel, (double)s.launch, (double)s.vec,    (double)s.th,  (double)s.tw,
                         (double)s.rows,   (double)s.chunks, (double)s.units,  (double)s.grid};
    for (int i = 0; i < 9; ++i) out[i] = v[i];
}
}
