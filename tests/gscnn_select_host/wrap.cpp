// C entry points over csrc/gscnn_select.h for tests/test_gscnn_select_host.py (ctypes) and sweep_main.cpp: every selector with its
// operands flattened -- a pointer is its 64-bit value, 0 an absent operand -- its result flattened to doubles, the constants, the
// grid helper, the small-wgrad block rule, the two workspace sizes and the name the launchers note for each kernel value.
#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/gscnn_select.h"

namespace {
const void *ptr(long long v) { return (const void *)(uintptr_t)v; }
// out: kernel, why, grid, grid2, threads, lds, raise_lds, sw_blocks, sw_per_block, nsx, nsy, total, ws_off[3], sh, sw
void flat(const GsSel &c, double *out)
{
    const double v[17] = {(double)c.kernel, (double)c.why, (double)c.grid, (double)c.grid2, (double)c.threads, (double)c.lds, (double)c.raise_lds,
                          (double)c.sw_blocks, (double)c.sw_per_block, (double)c.nsx, (double)c.nsy, (double)c.total, (double)c.ws_off[0],
                          (double)c.ws_off[1], (double)c.ws_off[2], c.sh, c.sw};
    for (int i = 0; i < 17; ++i) out[i] = v[i];
}
}  // namespace

extern "C" {
const char *gs_name(int k) { return gs_kernel_name(k); }
int gs_refused(void) { return GS_REFUSED; }
long long gs_const(int i)
{
    const long long v[] = {GS_SL_MAXC, GS_SW_CH, GS_SW_PIX_PER_BLOCK, GS_SW_MAX_BLOCKS, GS_SC_SEG, GS_SC_ROWS, GS_SC_RING, GS_SC_THREADS_64, GS_THREADS,
                           GS_SC_LDS_LIMIT, GS_GC_PIX, GS_GC_PIX_WIDE, GS_GC_WIDE_C, GS_MFMA_PIX, GS_MFMA_WAVES, GS_CANNY_GRAD_BYTES, GS_CANNY_MAG_BYTES,
                           GS_CANNY_STATE_BYTES, GS_CANNY_SLACK, GS_CAP_GATED_MFMA, GS_CAP_POINTWISE_SMALL, GS_CAP_GATED, GS_CAP_EDGE_ATTENTION,
                           GS_CAP_EDGE_ASPP, GS_CAP_CANNY, GS_CAP_SMALL_LINEAR, GS_CAP_GATE_MIX_BWD, GS_CAP_EDGE_ATTENTION_BWD, GS_CAP_RANK1_ADD};
    return i >= 0 && i < (int)(sizeof(v) / sizeof(v[0])) ? v[i] : -1;
}
int gs_sl_template(int i) { return i >= 0 && i < (int)(sizeof(GS_SL_TEMPLATES) / sizeof(GS_SL_TEMPLATES[0])) ? GS_SL_TEMPLATES[i] : -1; }
unsigned gs_grid_of(long long total, int cap) { return gs_grid(total, cap); }
int gs_dtype_is_ok(int d) { return gs_dtype_ok(d); }
int gs_gated_pix_of(int C) { return gs_gated_pix(C); }
// small_wgrad's block rule at npix >= 1 (the workspace function and the selector never ask it below)
int gs_sw_blocks(long long npix, long long *per_block) { return gs_small_wgrad_blocks(npix, per_block); }
unsigned long long gs_ws_canny(int N, int H, int W) { return gs_canny_workspace(N, H, W); }
unsigned long long gs_ws_small_wgrad(int Ca, int Cb, long long npix) { return gs_small_wgrad_workspace(Ca, Cb, npix); }

void gs_sel_gated_conv(int dtype, long long feat, int ldf, long long out_, int ldo, long long npix, int C, int mfma, double *out)
{
    flat(gs_gated_conv(dtype, ptr(feat), ldf, ptr(out_), ldo, npix, C, mfma != 0), out);
}
void gs_sel_edge_attention(int dtype, long long cs, int ldc, long long npix, double *out) { flat(gs_edge_attention(dtype, ptr(cs), ldc, npix), out); }
void gs_sel_edge_aspp(int dtype, long long w, long long scale, long long shift, long long y, int ldy, int N, int H, int W, int Ho, int Wo, int C,
                      double *out)
{
    flat(gs_edge_aspp(dtype, ptr(w), ptr(scale), ptr(shift), ptr(y), ldy, N, H, W, Ho, Wo, C), out);
}
void gs_sel_canny(int N, int H, int W, int sweeps, double *out) { flat(gs_canny(N, H, W, sweeps), out); }
void gs_sel_canny_continue(int N, int H, int W, int sweeps, double *out) { flat(gs_canny_continue(N, H, W, sweeps), out); }
void gs_sel_conv3x3_small(long long x, int ldx, long long w, long long res, int ldres, long long y, int ldy, int N, int H, int W, int C, double *out)
{
    flat(gs_conv3x3_small(ptr(x), ldx, ptr(w), ptr(res), ldres, ptr(y), ldy, N, H, W, C), out);
}
void gs_sel_pointwise_small(long long x, int ldx, long long y, int ldy, long long npix, int Cin, int Cout, double *out)
{
    flat(gs_pointwise_small(ptr(x), ldx, ptr(y), ldy, npix, Cin, Cout), out);
}
void gs_sel_small_linear(int x_dtype, int ldx, int Cin, int y_dtype, int ldy, int Cout, long long npix, long long mask, int ldm, double *out)
{
    flat(gs_small_linear(x_dtype, ldx, Cin, y_dtype, ldy, Cout, npix, ptr(mask), ldm), out);
}
void gs_sel_small_wgrad(int a_dtype, int lda, int Ca, int b_dtype, int ldb, int Cb, long long npix, double *out)
{
    flat(gs_small_wgrad(a_dtype, lda, Ca, b_dtype, ldb, Cb, npix), out);
}
void gs_sel_gate_mix_bwd(int feat_dtype, int C, long long npix, double *out) { flat(gs_gate_mix_bwd(feat_dtype, C, npix), out); }
void gs_sel_edge_attention_bwd(int dtype, int ldc, long long npix, double *out) { flat(gs_edge_attention_bwd(dtype, ldc, npix), out); }
void gs_sel_rank1_add(int dtype, long long y, int ldy, long long w, int C, long long npix, double *out)
{
    flat(gs_rank1_add(dtype, ptr(y), ldy, ptr(w), C, npix), out);
}
}
