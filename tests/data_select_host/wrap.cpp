// C entry points over csrc/data_select.h for tests/test_cifar_loader_host.py (ctypes) and sweep_main.cpp: the selector with its
// output pointer flattened to its 64-bit value and its result flattened to doubles, the predicates, the constants and the name the
// launcher notes for each kernel value.
#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/data_select.h"

namespace {
const void *ptr(long long v) { return (const void *)(uintptr_t)v; }
}  // namespace

extern "C" {
const char *ds_name(int k) { return data_kernel_name(k); }
int ds_count(void) { return DATA_COUNT; }
long long ds_const(int i)
{
    const long long v[] = {DATA_TPB, DATA_SIDE, DATA_CH, DATA_PIXELS, DATA_PAD, DATA_VEC_BYTES, DATA_MAX_ELEMS, KD_CIFAR_NCHW, KD_CIFAR_NHWC};
    return i >= 0 && i < (int)(sizeof(v) / sizeof(v[0])) ? v[i] : -1;
}
int ds_dtype_ok(int dtype) { return data_dtype_ok(dtype); }
int ds_layout_ok(int layout) { return data_layout_ok(layout); }
int ds_shape_ok(int layout, int B, int ld) { return data_shape_ok(layout, B, ld); }
long long ds_elems(int layout, int B, int ld) { return data_elems(layout, B, ld); }
// out: kernel, vec, elems, items, grid
void ds_select(int dtype, int layout, long long out_ptr, int B, int ld, double *out)
{
    const DataSel s = data_select(dtype, layout, ptr(out_ptr), B, ld);
    const double v[5] = {(double)s.kernel, (double)s.vec, (double)s.elems, (double)s.items, (double)s.grid};
    for (int i = 0; i < 5; ++i) out[i] = v[i];
}
}
