// C entry points over csrc/seg_data_select.h for tests/test_seg_data_select_host.py (ctypes) and sweep_main.cpp: the three selectors
// with their pointers flattened to 64-bit values and their results flattened to doubles, the predicates, the constants and the name
// the launchers note for each kernel value.
#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/seg_data_select.h"

namespace {
const void *ptr(long long v) { return (const void *)(uintptr_t)v; }
}  // namespace

extern "C" {
const char *ss_name(int k) { return seg_kernel_name(k); }
int ss_count(void) { return SEG_COUNT; }
long long ss_const(int i)
{
    const long long v[] = {SEG_TPB, SEG_TX, SEG_TY, SEG_CH, SEG_HDR, SEG_TAPS, SEG_ENTRY, SEG_CAP_C, SEG_CAP_R, SEG_MAX_RADIUS, SEG_JITTER_PIXELS,
                           SEG_VEC_BYTES, SEG_MAX_SIDE, SEG_MAX_BATCH, KD_SEG_NCHW, KD_SEG_NHWC, SK_CROP_1, SK_JITTER_1, SK_FINISH_0};
    return i >= 0 && i < (int)(sizeof(v) / sizeof(v[0])) ? v[i] : -1;
}
int ss_dtype_ok(int dtype) { return seg_dtype_ok(dtype); }
int ss_layout_ok(int layout) { return seg_layout_ok(layout); }
int ss_side_ok(int v) { return seg_side_ok(v); }
int ss_batch_ok(int B) { return seg_batch_ok(B); }
long long ss_row_words(int S) { return seg_row_words(S); }
long long ss_jitter_workspace(int B) { return (long long)seg_jitter_workspace(B); }
// out: kernel, store, gx, gy, gz
void ss_crop(long long img_out, long long mask_out, int B, int S, double *out)
{
    const SegCropSel s = seg_crop_select(ptr(img_out), ptr(mask_out), B, S);
    const double v[5] = {(double)s.kernel, (double)s.store, (double)s.gx, (double)s.gy, (double)s.gz};
    for (int i = 0; i < 5; ++i) out[i] = v[i];
}
// out: kernel, pixels, chunks, gx, gy
void ss_jitter(long long img, int B, int S, double *out)
{
    const SegJitterSel s = seg_jitter_select(ptr(img), B, S);
    const double v[5] = {(double)s.kernel, (double)s.pixels, (double)s.chunks, (double)s.gx, (double)s.gy};
    for (int i = 0; i < 5; ++i) out[i] = v[i];
}
// out: kernel, vec, src_vec, gx, gy, gz
void ss_finish(int dtype, int layout, int blur, long long img, long long mask, long long o, long long mask_out, int B, int H, int W, int ld, double *out)
{
    const SegFinishSel s = seg_finish_select(dtype, layout, blur, ptr(img), ptr(mask), ptr(o), ptr(mask_out), B, H, W, ld);
    const double v[6] = {(double)s.kernel, (double)s.vec, (double)s.src_vec, (double)s.gx, (double)s.gy, (double)s.gz};
    for (int i = 0; i < 6; ++i) out[i] = v[i];
}
}
