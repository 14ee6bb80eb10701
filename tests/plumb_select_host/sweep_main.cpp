// Stand-alone walk of the plumbing selection (csrc/plumb_select.h through wrap.cpp) for a sanitizer build: `make sweep` compiles this
// with -fsanitize=address,undefined and runs it.  Every selector over dtypes, base offsets, leading dimensions and shapes on both
// sides of every gate -- rows around the chunk caps, work items around the grid caps, a wave count above the 32-bit grid -- and each
// answer held to totality: a known kernel or PLUMB_REFUSED, grids of at least one block in every dimension, plans inside the
// workspace the header itself reports.
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/plumb_select.h"

extern "C" {
const char *ps_name(int k);
unsigned ps_grid(long long total, int cap);
void ps_geom(int h, int w, int H, int W, int align_corners, float *out);
int ps_cs_chunks(long long rows);
unsigned long long ps_ws_channel_sums(int groups, long long rows, int C);
unsigned long long ps_ws_bn_sums_finish(int rows, int C);
unsigned long long ps_ws_maxpool_bwd(int N, int H, int W, int C);
unsigned long long ps_ws_upsample_bwd(int N, int H, int W, int C, int Ho, int Wo);
unsigned long long ps_ws_stem_wgrad(int N, int H, int W);
unsigned long long ps_ws_image_pool(int N, int Cin, int Cout);
void ps_stem_conv(int dtype, int N, int H, int W, double *out);
void ps_stem_conv_pool(int N, int H, int W, double *out);
void ps_maxpool(int dtype, int N, int H, int W, int C, double *out);
void ps_upsample(long long x, int x_dtype, int ldx, long long y, int y_dtype, int ldy, int N, int H, int W, int C, int Ho, int Wo, int align_corners,
                 double *out);
void ps_image_pool(int dtype, int N, int H, int W, int Cin, int Cout, double *out);
void ps_image_pool_sums(int dtype, int N, int H, int W, int Cin, int Cout, double *out);
void ps_bn_fold(int C, double *out);
void ps_copy_cast(long long d_sC, int N, int C, long long P, double *out);
void ps_relu_bn_bwd(int dtype, long long M, int C, double *out);
void ps_channel_sums(int dtype, long long g, int ldg, long long sub, int ldsub, long long a, int lda, int groups, long long rows, int C, double *out);
void ps_bn_sums_finish(int rows, int C, double *out);
void ps_bn_eval_param_grads(int C, double *out);
void ps_maxpool_bwd(int dtype, long long x, int ldx, long long gy, int ldgy, long long gx, int ldgx, int N, int H, int W, int C, long long workspace,
                    unsigned long long workspace_bytes, double *out);
void ps_upsample_bwd(long long gy, int gy_dtype, int ldgy, long long gx, int gx_dtype, int ldgx, int N, int H, int W, int C, int Ho, int Wo,
                     int align_corners, long long workspace, double *out);
void ps_zero_insert(int dtype, int N, int C, int Hy, int Wy, double *out);
void ps_broadcast_add(int dtype, int N, long long HW, int C, double *out);
void ps_stem_wgrad(int dtype, long long dy, int ld_dy, int N, int H, int W, double *out);
void ps_direct_wgrad(int K, int Cg, double *out);
void ps_bn2d_fwd(int training, int C, double *out);
void ps_bn2d_bwd(int training, int C, double *out);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "sweep_main.cpp:%d: %s\n", __LINE__, #c); abort(); } } while (0)
enum { KERNEL, GX, GY, GZ, G2X, G2Y, G2Z, CHUNKS, LC, CBLOCKS, PER, VEC, FLAT4, TWO_PASS, WS0, WS1, WS2, BLOCKS, HO, WO, NGX, NSEG, SH, SW, OH, OW, NOUT };

static long long n_calls = 0;
// a kernel in [lo, hi] (or PLUMB_REFUSED where the entry point may refuse) and grids of at least one block in every dimension
static void total(const double *o, int lo, int hi, bool may_refuse = false)
{
    ++n_calls;
    const int k = (int)o[KERNEL];
    if (may_refuse && k == PLUMB_REFUSED) return;
    CHECK(k >= lo && k <= hi && ps_name(k) && strlen(ps_name(k)) > 0);
    for (int i = GX; i <= G2Z; ++i) CHECK(o[i] >= 1 && o[i] <= 4294967295.0);
}
static double ceil_div(double a, double b) { return (double)(((long long)a + (long long)b - 1) / (long long)b); }

int main()
{
    double o[NOUT];
    for (int k = 0; k < PLUMB_REFUSED; ++k) {
        CHECK(ps_name(k) && strlen(ps_name(k)) > 0);
        for (int j = 0; j < k; ++j) CHECK(strcmp(ps_name(j), ps_name(k)) != 0);
    }
    CHECK(!ps_name(PLUMB_REFUSED) && !ps_name(-1));

    const long long base = 0x10000;
    const int caps[] = {PLUMB_CAP_TRUNK, PLUMB_CAP_BWD, PLUMB_CAP_SMALL, PLUMB_CAP_COPY};
    for (int cap : caps) for (long long d : {-256LL, -1LL, 0LL, 1LL, 1LL << 40}) {
        const long long items = (long long)cap * 256 + d;
        const unsigned g = ps_grid(items, cap);
        CHECK(g >= 1 && g <= (unsigned)cap && (g == (unsigned)cap || (long long)g * 256 >= items));
        ++n_calls;
    }
    CHECK(ps_grid(-5, 8) == 1 && ps_grid(0, 8) == 1);

    // ---- channel sums: groups x rows x C x dtype x the three operands' presence, base offset and leading dimension
    for (int groups : {1, 2, 16, 64}) for (long long rows : {1LL, 511LL, 512LL, 513LL, 8200LL, 70000LL, 524287LL, 524288LL, 524289LL, 1LL << 40})
    for (int C : {3, 8, 19, 32, 33, 64, 72, 128, 136, 256, 264, 512}) for (int dt = 0; dt < 2; ++dt) for (int off : {0, 2, 4, 16})
    for (int pad : {0, 1, 8, 16}) for (int ops = 0; ops < 4; ++ops) {
        const int ld = C + pad, es = dt ? 2 : 4;
        ps_channel_sums(dt, base + off, ld, ops & 1 ? base : 0, C, ops & 2 ? base + off : 0, ld, groups, rows, C, o);
        total(o, PK_CS_F32_1, PK_CS_BF16_8);
        const bool vec = C % 8 == 0 && off % 16 == 0 && (ld * es) % 16 == 0 && (!(ops & 1) || (C * es) % 16 == 0);
        CHECK((int)o[KERNEL] == PK_CS_F32_1 + 2 * dt + vec && o[VEC] == vec);
        const int nvec = vec ? C / 8 : C;
        CHECK(o[LC] >= 4 && o[LC] <= 32 && o[CBLOCKS] * o[LC] >= nvec && (o[CBLOCKS] - 1) * o[LC] < nvec);
        CHECK(o[CHUNKS] >= 1 && o[CHUNKS] <= ps_cs_chunks(rows) && o[CHUNKS] <= rows && ps_cs_chunks(rows) <= PLUMB_CS_MAX_CHUNKS);
        CHECK(o[GX] == o[CHUNKS] && o[GY] == o[CBLOCKS] && o[GZ] == groups && o[G2X] == groups * ceil_div(C, 16));
        CHECK((double)groups * o[CHUNKS] * 2 * C * 4 <= (double)ps_ws_channel_sums(groups, rows, C));
    }

    // ---- the finishing stage of the conv epilogue's sums
    for (int rows : {1, 255, 256, 257, 1000, 16383, 16384, 16385, 1 << 22, 0x7fffffff}) for (int C : {1, 8, 24, 256, 4096}) {
        ps_bn_sums_finish(rows, C, o);
        total(o, PK_BNS_STAGE_64, PK_CS_FINISH);
        const bool staged = o[KERNEL] != PK_CS_FINISH;
        CHECK(staged == (rows > PLUMB_BNS_DIRECT_ROWS) && o[G2X] == ceil_div(C, 16) && o[GX] == o[G2X]);
        if (staged) CHECK((o[PER] == 64 || o[PER] == 256) && o[CHUNKS] * o[PER] >= rows && (o[CHUNKS] - 1) * o[PER] < rows && o[GY] == o[CHUNKS]);
        else CHECK(o[PER] == 0 && o[CHUNKS] == rows && o[GY] == 1);
        CHECK((staged ? o[CHUNKS] * 2 * C * 4 : 0) <= (double)ps_ws_bn_sums_finish(rows, C));
    }

    // ---- the two resampling directions and the two pools: shapes x dtypes x views
    const int ext[] = {1, 2, 7, 33, 64, 67, 128, 1024};
    for (int N : {1, 3}) for (int C : {1, 8, 19, 256}) for (int h : ext) for (int w : ext) for (int H : ext) for (int W : ext) for (int ac = 0; ac < 2; ++ac)
    for (int v = 0; v < 16; ++v) {
        const int xdt = v & 1, ydt = (v >> 1) & 1, off = v & 4 ? 4 : 0, pad = v & 8 ? 13 : 0;
        ps_upsample(base, xdt, C, base + off, ydt, C + pad, N, h, w, C, H, W, ac, o);
        total(o, PK_UP_F32_F32_1, PK_UP_FLAT4_BF16);
        const bool vec = C % 8 == 0 && !off && ((C + pad) * (ydt ? 2 : 4)) % 16 == 0 && (C * (xdt ? 2 : 4)) % 16 == 0;
        CHECK(o[VEC] == vec && !(o[VEC] && o[FLAT4]) && (!o[FLAT4] || (!ydt && !pad && !off && ((long long)W * C) % 4 == 0)));
        CHECK((int)o[KERNEL] == (o[FLAT4] ? PK_UP_FLAT4_F32 + xdt : PK_UP_F32_F32_1 + 4 * xdt + 2 * ydt + vec));
        CHECK(o[GX] * 256 * (o[FLAT4] ? 4 : vec ? 8 : 1) >= (double)W * C && o[GY] * PLUMB_UP_RO >= H && o[GZ] == N);
        CHECK(o[SH] >= 0 && o[SW] >= 0 && (ac ? o[OH] == 0 && o[OW] == 0 : o[OH] >= -0.5 && o[OW] >= -0.5));
        ps_upsample_bwd(base + off, xdt, C + pad, base, ydt, C, N, h, w, C, H, W, ac, v & 8 ? base + 8 : base, o);
        total(o, PK_UPB_F32_F32_1, PK_UPB_BF16_BF16_8);
        const bool bvec = C % 8 == 0 && !off && ((C + pad) * (xdt ? 2 : 4)) % 16 == 0 && (C * (ydt ? 2 : 4)) % 16 == 0 && !(v & 8);
        CHECK((int)o[KERNEL] == PK_UPB_F32_F32_1 + 4 * xdt + 2 * ydt + bvec);
        CHECK(o[GX] * 256 * (bvec ? 8 : 1) >= (double)w * C && o[GX] == o[G2X] && o[GY] == H && o[G2Y] == h && o[GZ] == N && o[G2Z] == N);
        CHECK((double)N * H * w * C * 4 <= (double)ps_ws_upsample_bwd(N, h, w, C, H, W));     // the pass along W writes (N, Ho, W, C) floats
        if (ac || v >= 2) continue;
        float g[4];
        ps_geom(h, w, H, W, 0, g);
        CHECK(g[0] == (float)h / (float)H && g[1] == (float)w / (float)W);
        const int dt = v & 1, Cp = C % 8 ? 8 : C;
        ps_maxpool(dt, N, h, w, Cp, o);
        total(o, PK_MAXPOOL_F32 + dt, PK_MAXPOOL_F32 + dt);
        CHECK(o[HO] == (h - 1) / 2 + 1 && o[WO] == (w - 1) / 2 + 1 && o[GX] * 256 >= o[WO] * (Cp / 8) && o[GY] == o[HO] && o[GZ] == N);
        const unsigned long long need = ps_ws_maxpool_bwd(N, h, w, C);
        for (int ws = 0; ws < 5; ++ws) {      // absent, one byte short, 4-B-misaligned, exact, exact at an 8-B offset
            const long long p = ws == 0 ? 0 : ws == 2 ? base + 4 : ws == 4 ? base + 8 : base;
            ps_maxpool_bwd(dt, base, C, base, C, base, C + H % 2, N, h, w, C, p, ws == 1 ? need - 1 : need, o);
            total(o, PK_MP_ARGMAX_F32, PK_MPB_BF16_8);
            const bool pv = C % 8 == 0 && ((C + H % 2) * (dt ? 2 : 4)) % 16 == 0, two = pv && ws >= 3;
            CHECK(o[TWO_PASS] == two && (int)o[KERNEL] == (two ? PK_MP_ARGMAX_F32 + dt : PK_MPB_F32_1 + 2 * dt + pv));
            CHECK(o[G2X] * 256 * (pv ? 8 : 1) >= (double)w * C && o[G2Y] == h && o[G2Z] == N);
            if (two) CHECK(o[GX] * 256 * 8 >= o[WO] * C && o[GY] == o[HO] && (double)N * o[HO] * o[WO] * (C / 8) * 8 <= (double)need);
        }
    }

    // ---- the flat grid-stride kernels around their caps, the copy at its 2^20 blocks
    for (int dt = 0; dt < 2; ++dt) for (long long d : {-256LL, -1LL, 0LL, 1LL}) for (int C : {8, 64}) {
        const long long items = (long long)PLUMB_CAP_BWD * 256 + d;
        ps_relu_bn_bwd(dt, items, C, o);
        total(o, PK_RELU_BN_BWD_F32 + dt, PK_RELU_BN_BWD_F32 + dt);
        CHECK(o[GX] <= PLUMB_CAP_BWD && (o[GX] == PLUMB_CAP_BWD || o[GX] * 256 >= (double)items * (C / 8)));
        ps_broadcast_add(dt, 2, items, C, o);
        total(o, PK_BCAST_ADD_F32 + dt, PK_BCAST_ADD_F32 + dt);
        CHECK(o[GX] == PLUMB_CAP_BWD);
        ps_copy_cast(dt ? 1 : 35, 1, 1, (long long)PLUMB_CAP_COPY * 256 + d, o);
        total(o, PK_COPY_CAST_CFAST, PK_COPY_CAST_PFAST);
        CHECK((int)o[KERNEL] == (dt ? PK_COPY_CAST_CFAST : PK_COPY_CAST_PFAST) && o[GX] == (d == -256 ? PLUMB_CAP_COPY - 1 : PLUMB_CAP_COPY));
        ps_zero_insert(dt, 2, C, 13, 19, o);
        total(o, PK_ZERO_INSERT_F32 + dt, PK_ZERO_INSERT_F32 + dt);
        CHECK(o[GX] * 256 >= 19.0 * (C / 8) && o[GY] == 13 && o[GZ] == 2);
    }

    // ---- image pooling: the three sub-arrays inside the workspace
    for (int dt = 0; dt < 2; ++dt) for (int N : {1, 3, 64}) for (int Cin : {8, 64, 264, 4096}) for (int Cout : {8, 256, 264}) for (int HW : {1, 60, 128, 8192 * 256 + 1}) {
        const double ws = (double)ps_ws_image_pool(N, Cin, Cout);
        for (int sums = 0; sums < 2; ++sums) {
            if (sums) ps_image_pool_sums(dt, N, 1, HW, Cin, Cout, o);
            else ps_image_pool(dt, N, 1, HW, Cin, Cout, o);
            total(o, PK_GAP_PARTIAL_F32 + dt, PK_GAP_PARTIAL_F32 + dt);
            CHECK(o[WS0] == 0 && o[WS0] + 4.0 * PLUMB_GAP_CHUNKS * N * Cin <= o[WS1] && o[WS1] + 4.0 * N * Cin <= o[WS2] && o[WS2] + 4.0 * N * Cout <= ws);
            CHECK(o[G2X] <= PLUMB_CAP_TRUNK && (sums ? o[GX] * 32 >= Cin && o[GY] == N : o[GX] == PLUMB_GAP_CHUNKS && o[GY] * 256 >= Cin && o[GZ] == N));
        }
    }

    // ---- the stem: persistent grids, the work-item cap, the refusal above a 2^31 - 1 block grid
    for (int dt = 0; dt < 2; ++dt) for (int N : {1, 3}) for (int H : {1, 5, 767, 768, 769, 1024}) for (int W : {1, 16, 21, 256, 257, 2048}) {
        ps_stem_conv(dt, N, H, W, o);
        total(o, PK_STEM_CONV_F32, PK_STEM_CONV_MFMA);
        CHECK((int)o[KERNEL] == (dt ? PK_STEM_CONV_MFMA : PK_STEM_CONV_F32) && (dt ? o[GX] <= PLUMB_STEM_MFMA_MAX_BLOCKS && o[NGX] * 16 >= W : o[GX] * 64 >= (double)N * H * W));
        for (int off : {0, 2, 16}) for (int ld : {64, 68, 72}) {
            ps_stem_wgrad(dt, base + off, ld, N, H, W, o);
            total(o, PK_STEM_WGRAD_MFMA, PK_STEM_WGRAD_BF16);
            CHECK((int)o[KERNEL] == (dt && off != 2 && ld != 68 ? PK_STEM_WGRAD_MFMA : PK_STEM_WGRAD_F32 + dt));
            CHECK(o[BLOCKS] == o[GX] && o[BLOCKS] <= PLUMB_STEM_MAX_BLOCKS && o[BLOCKS] * 64 * 27 * 4 <= (double)ps_ws_stem_wgrad(N, H, W));
        }
    }
    for (int N : {1, 2, 296204641, 0x7fffffff}) for (int H : {1, 17, 32, 33, 2048}) for (int W : {1, 37, 43, 393, 2048}) {
        ps_stem_conv_pool(N, H, W, o);
        total(o, PK_STEM_POOL, PK_STEM_POOL, true);
        const double waves = (double)N * o[NGX] * o[NSEG];
        CHECK(o[NGX] * PLUMB_SP_COLS >= o[WO] && o[NSEG] * PLUMB_SP_ROWS >= o[HO] && (o[KERNEL] == PLUMB_REFUSED) == (waves > 4.0 * 2147483647.0));
        if (o[KERNEL] != PLUMB_REFUSED) CHECK(o[GX] * 4 >= waves);
    }

    for (int C : {1, 8, 256, 600, 4096}) {
        ps_bn_fold(C, o); total(o, PK_BN_FOLD, PK_BN_FOLD); CHECK(o[GX] * 256 >= C);
        ps_bn_eval_param_grads(C, o); total(o, PK_BN_EVAL_PARAM_GRADS, PK_BN_EVAL_PARAM_GRADS); CHECK(o[GX] * 256 >= C);
        for (int tr = 0; tr < 2; ++tr) {
            ps_bn2d_fwd(tr, C, o); total(o, PK_BN2D_FWD_EVAL + tr, PK_BN2D_FWD_EVAL + tr); CHECK(o[GX] == C);
            ps_bn2d_bwd(tr, C, o); total(o, PK_BN2D_BWD_EVAL + tr, PK_BN2D_BWD_EVAL + tr); CHECK(o[GX] == C);
        }
        for (int Cg : {1, 3, 64}) { ps_direct_wgrad(C, Cg, o); total(o, PK_DCONV_WGRAD, PK_DCONV_WGRAD); CHECK(o[GX] == (double)C * Cg && o[G2X] == C); }
    }
    printf("plumb_select sweep: %lld calls walked through every selector, no finding\n", n_calls);
    return 0;
}
