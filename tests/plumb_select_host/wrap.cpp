// C entry points over csrc/plumb_select.h for tests/test_plumb_select_host.py (ctypes) and sweep_main.cpp: every selector with its
// operands flattened -- a pointer is its 64-bit value, 0 an absent operand -- its result flattened to doubles, the constants, the
// grid helper, the resampling geometry, the workspace sizes and the name the launchers note for each kernel value.
#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/plumb_select.h"

namespace {
const void *ptr(long long v) { return (const void *)(uintptr_t)v; }
// out: kernel, grid x y z, grid2 x y z, chunks, lc, cblocks, per, vec, flat4, two_pass, ws_off[3], blocks, Ho, Wo, ngx, nseg, sh, sw, oh, ow
void flat(const PlumbSel &c, double *out)
{
    const double v[26] = {(double)c.kernel, (double)c.grid.x, (double)c.grid.y, (double)c.grid.z, (double)c.grid2.x, (double)c.grid2.y, (double)c.grid2.z,
                          (double)c.chunks, (double)c.lc, (double)c.cblocks, (double)c.per, (double)c.vec, (double)c.flat4, (double)c.two_pass,
                          (double)c.ws_off[0], (double)c.ws_off[1], (double)c.ws_off[2], (double)c.blocks, (double)c.Ho, (double)c.Wo, (double)c.ngx,
                          (double)c.nseg, c.sh, c.sw, c.oh, c.ow};
    for (int i = 0; i < 26; ++i) out[i] = v[i];
}
}  // namespace

extern "C" {
const char *ps_name(int k) { return plumb_kernel_name(k); }
int ps_refused(void) { return PLUMB_REFUSED; }
long long ps_const(int i)
{
    const long long v[] = {PLUMB_SW_SEG, PLUMB_STEM_MAX_BLOCKS, PLUMB_STEM_MFMA_MAX_BLOCKS, PLUMB_SP_COLS, PLUMB_SP_ROWS, PLUMB_GAP_CHUNKS, PLUMB_UP_RO,
                           PLUMB_CS_ROWS, PLUMB_CS_MAX_CHUNKS, PLUMB_CS_BLOCKS, PLUMB_CS_MIN_CHUNKS, PLUMB_BNS_DIRECT_ROWS, PLUMB_BNS_LONG_ROWS,
                           PLUMB_BNS_PER, PLUMB_BNS_PER_LONG, PLUMB_CAP_TRUNK, PLUMB_CAP_BWD, PLUMB_CAP_SMALL, PLUMB_CAP_COPY};
    return i >= 0 && i < (int)(sizeof(v) / sizeof(v[0])) ? v[i] : -1;
}
unsigned ps_grid(long long total, int cap) { return plumb_grid(total, cap); }
int ps_vec_ok(long long p, int ld, int es) { return plumb_vec_ok(ptr(p), ld, es); }
int ps_dtype_ok(int d) { return plumb_dtype_ok(d); }
void ps_geom(int h, int w, int H, int W, int align_corners, float *out)
{
    const PlumbUpGeom g = plumb_up_geom(h, w, H, W, align_corners);
    out[0] = g.sh; out[1] = g.sw; out[2] = g.oh; out[3] = g.ow;
}
int ps_cs_chunks(long long rows) { return plumb_cs_chunks(rows); }

unsigned long long ps_ws_channel_sums(int groups, long long rows, int C) { return plumb_channel_sums_workspace(groups, rows, C); }
unsigned long long ps_ws_bn_sums_finish(int rows, int C) { return plumb_bn_sums_finish_workspace(rows, C); }
unsigned long long ps_ws_maxpool_bwd(int N, int H, int W, int C) { return plumb_maxpool_bwd_workspace(N, H, W, C); }
unsigned long long ps_ws_upsample_bwd(int N, int H, int W, int C, int Ho, int Wo) { return plumb_upsample_bwd_workspace(N, H, W, C, Ho, Wo); }
unsigned long long ps_ws_stem_wgrad(int N, int H, int W) { return plumb_stem_wgrad_workspace(N, H, W); }
unsigned long long ps_ws_image_pool(int N, int Cin, int Cout) { return plumb_image_pool_workspace(N, Cin, Cout); }

void ps_stem_conv(int dtype, int N, int H, int W, double *out) { flat(plumb_select_stem_conv(dtype, N, H, W), out); }
void ps_stem_conv_pool(int N, int H, int W, double *out) { flat(plumb_select_stem_conv_pool(N, H, W), out); }
void ps_maxpool(int dtype, int N, int H, int W, int C, double *out) { flat(plumb_select_maxpool(dtype, N, H, W, C), out); }
void ps_upsample(long long x, int x_dtype, int ldx, long long y, int y_dtype, int ldy, int N, int H, int W, int C, int Ho, int Wo, int align_corners,
                 double *out)
{
    flat(plumb_select_upsample(ptr(x), x_dtype, ldx, ptr(y), y_dtype, ldy, N, H, W, C, Ho, Wo, align_corners), out);
}
void ps_image_pool(int dtype, int N, int H, int W, int Cin, int Cout, double *out) { flat(plumb_select_image_pool(dtype, N, H, W, Cin, Cout), out); }
void ps_image_pool_sums(int dtype, int N, int H, int W, int Cin, int Cout, double *out) { flat(plumb_select_image_pool_sums(dtype, N, H, W, Cin, Cout), out); }
void ps_bn_fold(int C, double *out) { flat(plumb_select_bn_fold(C), out); }
void ps_copy_cast(long long d_sC, int N, int C, long long P, double *out) { flat(plumb_select_copy_cast(d_sC, N, C, P), out); }
void ps_relu_bn_bwd(int dtype, long long M, int C, double *out) { flat(plumb_select_relu_bn_bwd(dtype, M, C), out); }
void ps_channel_sums(int dtype, long long g, int ldg, long long sub, int ldsub, long long a, int lda, int groups, long long rows, int C, double *out)
{
    flat(plumb_select_channel_sums(dtype, ptr(g), ldg, ptr(sub), ldsub, ptr(a), lda, groups, rows, C), out);
}
void ps_bn_sums_finish(int rows, int C, double *out) { flat(plumb_select_bn_sums_finish(rows, C), out); }
void ps_bn_eval_param_grads(int C, double *out) { flat(plumb_select_bn_eval_param_grads(C), out); }
void ps_maxpool_bwd(int dtype, long long x, int ldx, long long gy, int ldgy, long long gx, int ldgx, int N, int H, int W, int C, long long workspace,
                    unsigned long long workspace_bytes, double *out)
{
    flat(plumb_select_maxpool_bwd(dtype, ptr(x), ldx, ptr(gy), ldgy, ptr(gx), ldgx, N, H, W, C, ptr(workspace), (size_t)workspace_bytes), out);
}
void ps_upsample_bwd(long long gy, int gy_dtype, int ldgy, long long gx, int gx_dtype, int ldgx, int N, int H, int W, int C, int Ho, int Wo,
                     int align_corners, long long workspace, double *out)
{
    flat(plumb_select_upsample_bwd(ptr(gy), gy_dtype, ldgy, ptr(gx), gx_dtype, ldgx, N, H, W, C, Ho, Wo, align_corners, ptr(workspace)), out);
}
void ps_zero_insert(int dtype, int N, int C, int Hy, int Wy, double *out) { flat(plumb_select_zero_insert(dtype, N, C, Hy, Wy), out); }
void ps_broadcast_add(int dtype, int N, long long HW, int C, double *out) { flat(plumb_select_broadcast_add(dtype, N, HW, C), out); }
void ps_stem_wgrad(int dtype, long long dy, int ld_dy, int N, int H, int W, double *out) { flat(plumb_select_stem_wgrad(dtype, ptr(dy), ld_dy, N, H, W), out); }
void ps_direct_wgrad(int K, int Cg, double *out) { flat(plumb_select_direct_wgrad(K, Cg), out); }
void ps_bn2d_fwd(int training, int C, double *out) { flat(plumb_select_bn2d_fwd(training, C), out); }
void ps_bn2d_bwd(int training, int C, double *out) { flat(plumb_select_bn2d_bwd(training, C), out); }
}
