// Stand-alone walk of the shape-stream selection (csrc/gscnn_select.h through wrap.cpp) for a sanitizer build: `make sweep` compiles
// this with -fsanitize=address,undefined and runs it.  Every selector over dtypes, base offsets, leading dimensions, channel counts
// and sizes on both sides of every gate -- zero and negative sizes, pixel counts around 2^31 and far beyond, work items around every
// grid cap, a conv3x3_small image of more workgroups than a 32-bit grid -- and each answer held to totality: a kernel of the entry
// point's own range on a grid of 1 .. cap workgroups that covers the work or sits at its cap, or GS_REFUSED with a reason.
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/gscnn_select.h"

extern "C" {
const char *gs_name(int k);
unsigned gs_grid_of(long long total, int cap);
int gs_sw_blocks(long long npix, long long *per_block);
unsigned long long gs_ws_canny(int N, int H, int W);
unsigned long long gs_ws_small_wgrad(int Ca, int Cb, long long npix);
void gs_sel_gated_conv(int dtype, long long feat, int ldf, long long out_, int ldo, long long npix, int C, int mfma, double *out);
void gs_sel_edge_attention(int dtype, long long cs, int ldc, long long npix, double *out);
void gs_sel_edge_aspp(int dtype, long long w, long long scale, long long shift, long long y, int ldy, int N, int H, int W, int Ho, int Wo, int C,
                      double *out);
void gs_sel_canny(int N, int H, int W, int sweeps, double *out);
void gs_sel_canny_continue(int N, int H, int W, int sweeps, double *out);
void gs_sel_conv3x3_small(long long x, int ldx, long long w, long long res, int ldres, long long y, int ldy, int N, int H, int W, int C, double *out);
void gs_sel_pointwise_small(long long x, int ldx, long long y, int ldy, long long npix, int Cin, int Cout, double *out);
void gs_sel_small_linear(int x_dtype, int ldx, int Cin, int y_dtype, int ldy, int Cout, long long npix, long long mask, int ldm, double *out);
void gs_sel_small_wgrad(int a_dtype, int lda, int Ca, int b_dtype, int ldb, int Cb, long long npix, double *out);
void gs_sel_gate_mix_bwd(int feat_dtype, int C, long long npix, double *out);
void gs_sel_edge_attention_bwd(int dtype, int ldc, long long npix, double *out);
void gs_sel_rank1_add(int dtype, long long y, int ldy, long long w, int C, long long npix, double *out);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "sweep_main.cpp:%d: %s\n", __LINE__, #c); abort(); } } while (0)
enum { KERNEL, WHY, GRID, GRID2, THREADS, LDS, RAISE, SW_BLOCKS, SW_PER_BLOCK, NSX, NSY, TOTAL, WS0, WS1, WS2, SH, SW, NOUT };

static long long n_calls = 0;
// a kernel in [lo, hi] on 1 .. cap workgroups of 256 (512) threads, or a refusal that says why; -> true for a kernel
static bool total(const double *o, int lo, int hi, double cap)
{
    ++n_calls;
    const int k = (int)o[KERNEL];
    if (k == GS_REFUSED) {
        CHECK(o[WHY] > GS_WHY_NONE && o[WHY] <= GS_WHY_TOO_LARGE && o[GRID] == 0 && o[THREADS] == 0);
        return false;
    }
    CHECK(k >= lo && k <= hi && gs_name(k) && strlen(gs_name(k)) > 0 && o[WHY] == GS_WHY_NONE);
    CHECK(o[GRID] >= 1 && o[GRID] <= cap && o[GRID2] >= 1 && o[GRID2] <= cap);
    CHECK(o[THREADS] == (k == GS_CONV3X3_64 ? GS_SC_THREADS_64 : GS_THREADS));
    return true;
}
// the grid covers `items` threads' worth of work or sits at its cap
static void covers(const double *o, double items, double cap) { CHECK(o[GRID] == cap || o[GRID] * GS_THREADS >= items); }

int main()
{
    double o[NOUT];
    for (int k = 0; k < GS_REFUSED; ++k) {
        CHECK(gs_name(k) && strlen(gs_name(k)) > 0);
        for (int j = 0; j < k; ++j) CHECK(strcmp(gs_name(j), gs_name(k)) != 0);
    }
    CHECK(!gs_name(GS_REFUSED) && !gs_name(-1));

    const long long base = 0x10000, big = 1LL << 31, huge = 1LL << 62, most = INT64_MAX;
    const long long sizes[] = {-most, -1, 0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, big - 1, big, big + 1, 1LL << 40, huge, most};
    const int caps[] = {GS_CAP_GATED_MFMA, GS_CAP_POINTWISE_SMALL, GS_CAP_GATED, GS_CAP_EDGE_ATTENTION, GS_CAP_EDGE_ASPP, GS_CAP_CANNY,
                        GS_CAP_SMALL_LINEAR, GS_CAP_GATE_MIX_BWD, GS_CAP_EDGE_ATTENTION_BWD, GS_CAP_RANK1_ADD};
    for (int cap : caps) {
        for (long long d : {-256LL, -1LL, 0LL, 1LL, 1LL << 40}) {
            const long long items = (long long)cap * GS_THREADS + d;
            const unsigned g = gs_grid_of(items, cap);
            CHECK(g >= 1 && g <= (unsigned)cap && (g == (unsigned)cap || (long long)g * GS_THREADS >= items));
            ++n_calls;
        }
        for (long long t : sizes) CHECK(gs_grid_of(t, cap) >= 1 && gs_grid_of(t, cap) <= (unsigned)cap);
    }

    // ---- kd_gated_conv: dtype x C x base offset x leading dimension x the switch x size
    for (int dt = -1; dt < 3; ++dt) for (int C : {0, 8, 12, 16, 32, 64}) for (int off : {0, 2, 8, 16}) for (int pad : {0, 1, 4, 8, 0x7fffffff - 64})
    for (int mfma = 0; mfma < 2; ++mfma) for (long long npix : sizes) {
        gs_sel_gated_conv(dt, base + off, C + pad, base, C + pad, npix, C, mfma, o);
        const bool ran = total(o, GS_GATED_F32_8, GS_GATED_MFMA_32, GS_CAP_GATED);
        const int es = dt == 1 ? 2 : 4;
        const bool ok = npix > 0 && (dt == 0 || dt == 1) && (C == 8 || C == 16 || C == 32) && off % 16 == 0 && ((long long)(C + pad) * es) % 16 == 0;
        CHECK(ran == ok);
        if (!ran) continue;
        const bool matrix = o[KERNEL] >= GS_GATED_MFMA_8;
        CHECK(matrix == (mfma && dt == 1));
        if (matrix) { CHECK(o[GRID] <= GS_CAP_GATED_MFMA); covers(o, (double)npix / GS_MFMA_PIX * 64, GS_CAP_GATED_MFMA); }
        else covers(o, (double)npix / (C >= 32 ? GS_GC_PIX_WIDE : GS_GC_PIX), GS_CAP_GATED);
    }

    // ---- kd_edge_attention / kd_edge_attention_bwd / kd_gate_mix_bwd
    for (int dt = -1; dt < 3; ++dt) for (int off : {0, 4, 16}) for (int ld : {-8, 0, 7, 8, 9, 12, 64}) for (long long npix : sizes) {
        gs_sel_edge_attention(dt, base + off, ld, npix, o);
        if (total(o, GS_EDGE_ATTENTION_F32, GS_EDGE_ATTENTION_BF16, GS_CAP_EDGE_ATTENTION)) {
            CHECK((int)o[KERNEL] == GS_EDGE_ATTENTION_F32 + dt && off % 16 == 0 && (ld * (dt ? 2 : 4)) % 16 == 0 && npix > 0);
            covers(o, (double)npix, GS_CAP_EDGE_ATTENTION);
        }
        gs_sel_edge_attention_bwd(dt, ld, npix, o);
        if (total(o, GS_EDGE_ATTENTION_BWD, GS_EDGE_ATTENTION_BWD, GS_CAP_EDGE_ATTENTION_BWD)) { CHECK(ld >= 8 && npix > 0 && (dt == 0 || dt == 1)); covers(o, (double)npix, GS_CAP_EDGE_ATTENTION_BWD); }
        gs_sel_gate_mix_bwd(dt, ld, npix, o);
        if (total(o, GS_GATE_MIX_BWD, GS_GATE_MIX_BWD, GS_CAP_GATE_MIX_BWD)) { CHECK(ld >= 1 && npix > 0 && (dt == 0 || dt == 1)); covers(o, (double)npix, GS_CAP_GATE_MIX_BWD); }
    }

    // ---- kd_edge_aspp: extents up to the largest int, whose product no 64-bit integer holds
    const int ext[] = {-1, 0, 1, 2, 7, 1024, 0x7fffffff};
    for (int dt = 0; dt < 2; ++dt) for (int N : {0, 1, 2, 0x7fffffff}) for (int H : ext) for (int W : {1, 9}) for (int Ho : ext) for (int Wo : ext)
    for (int C : {-8, 0, 8, 12, 256, 0x7ffffff8}) for (int off : {0, 4}) {
        const int ld = C > 0x7fffff00 ? C : C + 16;
        gs_sel_edge_aspp(dt, base, base, base + off, base, ld, N, H, W, Ho, Wo, C, o);
        const bool ran = total(o, GS_EDGE_ASPP_F32, GS_EDGE_ASPP_BF16, GS_CAP_EDGE_ASPP);
        CHECK(ran == (N > 0 && H > 0 && Ho > 0 && Wo > 0 && C > 0 && C % 8 == 0 && !off && ((long long)ld * (dt ? 2 : 4)) % 16 == 0));
        if (!ran) continue;
        covers(o, (double)N * Ho * Wo * (C / 8), GS_CAP_EDGE_ASPP);
        CHECK(o[SH] >= 0 && o[SW] >= 0 && (Ho > 1 || o[SH] == 0) && (Wo > 1 || o[SW] == 0));
    }

    // ---- kd_canny / kd_canny_continue: the three sections inside the workspace the header reports
    for (int N : {-1, 0, 1, 2, 4096}) for (int H : {-3, 0, 1, 9, 1024, 65536}) for (int W : {0, 1, 7, 1400, 65536}) for (int sweeps : {-1, 0, 1, 8}) {
        (void)gs_ws_canny(N, H, W);
        for (int cont = 0; cont < 2; ++cont) {
            if (cont) gs_sel_canny_continue(N, H, W, sweeps, o);
            else gs_sel_canny(N, H, W, sweeps, o);
            const bool ran = total(o, GS_CANNY, GS_CANNY_CONTINUE, GS_CAP_CANNY);
            CHECK(ran == (N > 0 && H > 0 && W > 0 && sweeps >= cont));
            if (!ran) continue;
            const double n = (double)N * H * W;
            CHECK((int)o[KERNEL] == GS_CANNY + cont && o[TOTAL] == n && o[WS0] == 0 && o[WS1] == n * GS_CANNY_GRAD_BYTES && o[WS2] == o[WS1] + n * GS_CANNY_MAG_BYTES);
            CHECK(o[WS2] + n * GS_CANNY_STATE_BYTES <= (double)gs_ws_canny(N, H, W));
            covers(o, n, GS_CAP_CANNY);
        }
    }

    // ---- kd_conv3x3_small: views, channel counts, and images up to more workgroups than a 32-bit grid
    for (int C : {0, 8, 16, 32, 48, 64}) for (int off : {0, 8, 16}) for (int pad : {-8, 0, 4, 8}) for (int res = 0; res < 3; ++res)
    for (int N : {0, 1, 3, 0x7fffffff}) for (int H : {-1, 1, 16, 17, 0x7fffffff}) for (int W : {0, 1, 256, 257, 0x7fffffff}) {
        gs_sel_conv3x3_small(base + off, C + pad, base, res ? base + (res == 2 ? 8 : 0) : 0, C, base + 64, C + pad, N, H, W, C, o);
        if (!total(o, GS_CONV3X3_16, GS_CONV3X3_64, 2147483647.0)) {
            const double blocks = (double)N * ((W + 255LL) / 256) * ((H + 15LL) / 16);
            CHECK((o[WHY] == GS_WHY_TOO_LARGE) == (N > 0 && H > 0 && W > 0 && (C == 16 || C == 32 || C == 64) && off % 16 == 0 && (pad == 0 || pad == 8) && res != 2 && blocks > 2147483647.0));
            continue;
        }
        CHECK((int)o[KERNEL] == (C == 64 ? GS_CONV3X3_64 : C == 32 ? GS_CONV3X3_32 : GS_CONV3X3_16) && res != 2 && off % 16 == 0);
        CHECK(o[NSX] * GS_SC_SEG >= W && (o[NSX] - 1) * GS_SC_SEG < W && o[NSY] * GS_SC_ROWS >= H && (o[NSY] - 1) * GS_SC_ROWS < H);
        CHECK(o[GRID] == (double)N * o[NSX] * o[NSY] && o[LDS] == GS_SC_RING * (GS_SC_SEG + 2) * (C == 64 ? 144 : C * 2) && o[RAISE] == (C != 16));
    }

    // ---- kd_pointwise_small
    for (int Cin : {8, 16, 32, 64, 128}) for (int Cout : {4, 8, 16, 32, 64}) for (int xoff : {0, 8, 16}) for (int yoff : {0, 2, 4, 8}) for (int ypad : {-4, 0, 2, 4, 12})
    for (long long npix : sizes) {
        gs_sel_pointwise_small(base + xoff, Cin + 16, base + yoff, Cout + ypad, npix, Cin, Cout, o);
        const bool ran = total(o, GS_POINTWISE_64_32, GS_POINTWISE_16_8, GS_CAP_POINTWISE_SMALL);
        CHECK(ran == (npix > 0 && Cin == 2 * Cout && Cin >= 16 && Cin <= 64 && xoff % 16 == 0 && yoff % 8 == 0 && ypad >= 0 && ypad % 4 == 0));
        if (ran) covers(o, (double)npix / GS_MFMA_PIX * 64, GS_CAP_POINTWISE_SMALL);
    }

    // ---- kd_small_linear / kd_small_wgrad: channel counts around every template and the limit, strides, the block rule
    for (int xdt = -1; xdt < 3; ++xdt) for (int ydt = 0; ydt < 3; ++ydt) for (int Cin : {0, 1, 33, 72, 73}) for (int Cout : {-1, 0, 1, 8, 9, 16, 17, 24, 25, 40, 41, 72, 73, 0x7fffffff})
    for (int pad : {-1, 0, 16}) for (int mask = 0; mask < 3; ++mask) for (long long npix : sizes) {
        gs_sel_small_linear(xdt, Cin + pad, Cin, ydt, Cout > 0x7fffff00 ? Cout : Cout + pad, Cout, npix, mask ? base : 0, mask == 2 ? Cout - 1 : Cout, o);
        const bool ran = total(o, GS_SMALL_LINEAR_8, GS_SMALL_LINEAR_72, GS_CAP_SMALL_LINEAR);
        CHECK(ran == (npix > 0 && (xdt == 0 || xdt == 1) && ydt < 2 && mask != 2 && Cin >= 1 && Cin <= GS_SL_MAXC && Cout >= 1 && Cout <= GS_SL_MAXC && pad >= 0));
        if (ran) {
            const int t = GS_SL_TEMPLATES[(int)o[KERNEL] - GS_SMALL_LINEAR_8];
            CHECK(Cout <= t && ((int)o[KERNEL] == GS_SMALL_LINEAR_8 || Cout > GS_SL_TEMPLATES[(int)o[KERNEL] - GS_SMALL_LINEAR_8 - 1]));
            covers(o, (double)npix, GS_CAP_SMALL_LINEAR);
        }
        if (mask) continue;
        gs_sel_small_wgrad(xdt, Cin + pad, Cin, ydt, Cout > 0x7fffff00 ? Cout : Cout + pad, Cout, npix, o);
        const bool wran = total(o, GS_SMALL_WGRAD, GS_SMALL_WGRAD, GS_SW_MAX_BLOCKS);
        CHECK(wran == (npix > 0 && (xdt == 0 || xdt == 1) && ydt < 2 && Cin >= 1 && Cin <= GS_SL_MAXC && Cout >= 1 && Cout <= GS_SL_MAXC && pad >= 0));
        const double ws = (double)gs_ws_small_wgrad(Cin, Cout, npix);
        CHECK((ws == 0) == (Cin < 1 || Cout < 1 || npix < 1));
        if (!wran) continue;
        long long pb = 0;
        CHECK(o[SW_BLOCKS] == gs_sw_blocks(npix, &pb) && o[SW_PER_BLOCK] == (double)pb && o[GRID] == o[SW_BLOCKS] && pb % GS_SW_CH == 0);
        CHECK((o[SW_BLOCKS] - 1) * (double)pb < (double)npix && o[SW_BLOCKS] * (double)pb >= (double)npix);
        CHECK(o[GRID2] * GS_THREADS >= Cin * Cout + Cout && ws == o[SW_BLOCKS] * (Cin * Cout + Cout) * 4);
    }

    // ---- kd_rank1_add
    for (int dt = -1; dt < 3; ++dt) for (int C : {-8, 0, 8, 12, 64, 0x7ffffff8}) for (int off : {0, 4, 16}) for (int woff : {0, 4}) for (int pad : {0, 2, 4, 16})
    for (long long npix : sizes) {
        gs_sel_rank1_add(dt, base + off, C > 0x7fffff00 ? C : C + pad, base + woff, C, npix, o);
        const bool ran = total(o, GS_RANK1_ADD_F32, GS_RANK1_ADD_BF16, GS_CAP_RANK1_ADD);
        const long long ld = C > 0x7fffff00 ? C : C + pad;
        CHECK(ran == (npix > 0 && C > 0 && (dt == 0 || dt == 1) && C % 8 == 0 && off % 16 == 0 && !woff && (ld * (dt ? 2 : 4)) % 16 == 0));
        if (ran) { CHECK((int)o[KERNEL] == GS_RANK1_ADD_F32 + dt); covers(o, (double)npix * (C / 8), GS_CAP_RANK1_ADD); }
    }
    printf("gscnn_select sweep: %lld calls walked through every selector, no finding\n", n_calls);
    return 0;
}
