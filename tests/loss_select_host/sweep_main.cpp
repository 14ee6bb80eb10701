// Stand-alone walk of the criterion selection (csrc/loss_select.h through wrap.cpp) for a sanitizer build: `make sweep` compiles
// this with -fsanitize=address,undefined and runs it.  Every selector over layouts, dtypes, base alignments and shapes on both sides
// of every gate -- extents of zero and of 2^30 for the resampling geometry, 1 and KD_MULTI_MAX operands -- and each answer held to
// what its kernel needs: the LDS it is launched with, the grid inside its partial arrays, the offsets inside the workspace.
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/loss_select.h"

extern "C" {
const char *ls_name(int k);
unsigned long long ls_workspace(int N, int C, long long P);
unsigned long long ls_topk_workspace(int N, int C, long long P);
void ls_pair(int kind, const long long *s, const long long *t, const long long *g, int N, int C, long long P, double *out);
void ls_mse(const long long *s, const long long *t, const long long *g, int N, int C, long long P, double *out);
void ls_whmse(int N, int C, long long P, double *out);
void ls_ce2d(const long long *x, int N, int C, long long P, double *out);
void ls_confusion(const long long *x, int N, int C, long long P, double *out);
void ls_up(int op, int N, int h, int w, int C, int H, int W, int align_corners, double *out);
void ls_topk(const long long *s, const long long *t, const long long *g, long long mask, long long workspace, int N, int C, long long P, double *out);
void ls_multi(const long long *s, const long long *ts, int nt, const long long *g, int smean, int N, int C, long long P, double *out);
void ls_scale(int dtype, long long n, double *out);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "sweep_main.cpp:%d: %s\n", __LINE__, #c); abort(); } } while (0)
enum { KERNEL, WHY, BLOCKS, LDS, CPR, NCHUNKS, CHUNKS, PER_CHUNK, AUX_OFF, SH, SW, OH, OW, NOUT };
enum { NCHW, CL, CSLICE, BSLICE, ROWS, NLAY };

// a view of layout `lay` at byte offset `off` from a 256-B aligned base
static void make(long long *v, int lay, int dt, int off, int N, int C, long long P)
{
    (void)N;
    const long long st[NLAY][3] = {{C * P, P, 1}, {C * P, 1, C}, {P * (C + 16), 1, C + 16}, {C * (P + 3), 1, C}, {C, 1, 0}};
    v[0] = 0x10000 + off; v[1] = dt; v[2] = st[lay][0]; v[3] = st[lay][1]; v[4] = st[lay][2];
}
static bool nhwc(const long long *v, int N, int C, long long P) { return v[3] == 1 && v[4] == C && (v[2] == (long long)C * P || N == 1); }

int main()
{
    long long n = 0;
    double o[NOUT];
    for (int k = 0; k < LOSS_REFUSED; ++k) {
        CHECK(ls_name(k) && strlen(ls_name(k)) > 0);
        for (int j = 0; j < k; ++j) CHECK(strcmp(ls_name(j), ls_name(k)) != 0);
    }
    CHECK(!ls_name(LOSS_REFUSED) && !ls_name(-1));

    const int offs[] = {0, 2, 4, 8, 16};
    for (int N : {1, 2}) for (int C : {1, 8, 9, 19, 32, 33, 53, 54, 64, 65}) for (long long P : {1LL, 8LL, 9LL, 35LL, 525001LL})
    for (int ls = 0; ls < NLAY; ++ls) for (int lg = 0; lg < NLAY; ++lg) for (int sdt = 0; sdt < 2; ++sdt) for (int tdt = 0; tdt < 2; ++tdt)
    for (int gdt = 0; gdt < 3; ++gdt) for (int off : offs) {
        long long s[5], t[5], g[5];
        make(s, ls, sdt, off, N, C, P); make(t, ls, tdt, 0, N, C, P); make(g, lg, gdt & 1, 0, N, C, P);
        const long long *gp = gdt == 2 ? nullptr : g;
        const long long rows = (long long)N * P, numel = rows * C;
        for (int kind = 0; kind < 3; ++kind) {
            ls_pair(kind, s, t, gp, N, C, P, o);
            CHECK(ls_name((int)o[KERNEL]) && o[BLOCKS] >= 1 && o[BLOCKS] <= LOSS_MAX_BLOCKS && (o[BLOCKS] == LOSS_MAX_BLOCKS || o[BLOCKS] * 256 >= rows));
            if (o[KERNEL] <= LK_PAIR_NHWC_LAST) {
                CHECK(o[LDS] == 2.0 * 256 * C * 4 && o[LDS] <= (double)LOSS_LDS_DEFAULT && nhwc(s, N, C, P) && nhwc(t, N, C, P) && (!gp || nhwc(g, N, C, P)));
                CHECK((int)o[KERNEL] == LK_PAIR_NHWC + 8 * kind + 4 * sdt + 2 * tdt + (gp ? gdt : sdt));
            } else {
                CHECK((int)o[KERNEL] == LK_PAIR_KLD + kind && o[LDS] == 0);
            }
        }
        const bool same = g[2] == s[2] && g[3] == s[3] && g[4] == s[4];
        ls_mse(s, t, gp, N, C, P, o);
        const bool vec = o[KERNEL] == LK_MSE_VEC_F32 || o[KERNEL] == LK_MSE_VEC_BF16;
        CHECK(vec || o[KERNEL] == LK_MSE_STRIDED);
        if (vec) CHECK(off % 16 == 0 && numel % 8 == 0 && sdt == tdt && (!gp || (gdt == sdt && same)) && (ls == NCHW || ls == CL) && (int)o[KERNEL] == LK_MSE_VEC_F32 + sdt);
        CHECK(o[BLOCKS] >= 1 && o[BLOCKS] <= LOSS_MAX_BLOCKS && o[LDS] == 0);
        for (long long ws : {0x20000LL, 0x20008LL}) for (long long mask : {0LL, 0x30000LL, 0x30004LL}) {
            ls_topk(s, t, gp, mask, ws, N, C, P, o);
            const int k = (int)o[KERNEL];
            CHECK(gp ? (k >= LK_TOPK_VEC_F32_CFAST && k <= LK_TOPK_GRAD) : k == LK_TOPK_NOGRAD);
            CHECK(o[CHUNKS] >= 1 && o[CHUNKS] <= LOSS_TOPK_MAX_CHUNKS && o[CHUNKS] <= P && o[CHUNKS] * o[PER_CHUNK] >= P);
            CHECK((long long)o[AUX_OFF] % 16 == 0 && o[AUX_OFF] + (double)N * C * 4 <= (double)ls_topk_workspace(N, C, P));
            if (k >= LK_TOPK_VEC_F32_CFAST && k <= LK_TOPK_VEC_BF16_PFAST) {
                CHECK(off % 16 == 0 && numel % 8 == 0 && sdt == tdt && gdt == sdt && same && (mask ? mask : ws + (long long)o[AUX_OFF]) % 16 == 0);
                CHECK(ls == CL ? (C % 8 == 0 && (k - LK_TOPK_VEC_F32_CFAST) % 2 == 0) : (ls == NCHW && P % 8 == 0 && (k - LK_TOPK_VEC_F32_CFAST) % 2 == 1));
            }
            if (gp) CHECK(o[BLOCKS] >= 1 && o[BLOCKS] <= LOSS_MAX_BLOCKS);
        }
        if (tdt == 0 && gdt == 0 && lg == 0) {
            ls_ce2d(s, N, C, P, o);
            CHECK(o[KERNEL] == LK_CE2D ? o[LDS] == 0 : ((int)o[KERNEL] == LK_CE2D_NHWC_F32 + sdt && nhwc(s, N, C, P) && o[LDS] == 256.0 * C * 4 && o[LDS] <= (double)LOSS_LDS_DEFAULT));
            ls_confusion(s, N, C, P, o);
            CHECK(o[LDS] <= (double)LOSS_LDS_DEFAULT && o[LDS] >= 4.0 * C * C);
            CHECK(o[KERNEL] == LK_CONFUSION ? o[LDS] == 4.0 * C * C : ((int)o[KERNEL] == LK_CONFUSION_NHWC_F32 + sdt && nhwc(s, N, C, P)));
            ls_whmse(N, C, P, o);
            CHECK(o[KERNEL] == LK_WHMSE && o[CHUNKS] >= 1 && o[CHUNKS] <= 64 && o[CHUNKS] * o[PER_CHUNK] >= P && o[BLOCKS] == o[CHUNKS] * ((C + 255) / 256) * N);
            CHECK(o[BLOCKS] * 8 <= o[AUX_OFF] && (long long)o[AUX_OFF] % 8 == 0 && o[AUX_OFF] + 4.0 * N <= (double)ls_workspace(N, C, P));
        }
        ++n;
    }

    // the five entry points on low-resolution logits: extents from 0 to 2^30, either alignment rule
    const int ext[] = {0, 1, 2, 7, 129, 300, 1 << 30};
    for (int op = LOSS_UP_CE2D; op <= LOSS_UP_METRICS; ++op) for (int C : {0, 1, 18, 19, 20, 23, 24, 25, 48, 49, 4096}) for (int N : {0, 1, 3})
    for (int h : ext) for (int w : ext) for (int H : ext) for (int W : ext) for (int ac = 0; ac < 2; ++ac) {
        ls_up(op, N, h, w, C, H, W, ac, o);
        const int bound = loss_up_max_classes((LossUpOp)op), cap = loss_up_max_blocks((LossUpOp)op);
        if (o[KERNEL] == LOSS_REFUSED) {
            CHECK(o[WHY] == LOSS_WHY_CLASSES ? C > bound : o[WHY] == LOSS_WHY_SPAN ? (N > 0 && h > 0 && w > 0 && C > 0 && H > 0 && W > 0) : (N < 1 || h < 1 || w < 1 || C < 1 || H < 1 || W < 1));
        } else {
            CHECK(C >= 1 && C <= bound && (int)o[KERNEL] == LK_CE2D_UP_0 + 2 * op + (C == 19) && o[WHY] == LOSS_WHY_NONE);
            CHECK((int)(255.f * (float)o[SW]) + 3 <= LOSS_UP_NW && o[SW] >= 0 && o[SH] >= 0);
            CHECK(o[BLOCKS] >= 1 && o[BLOCKS] <= cap && o[BLOCKS] <= o[NCHUNKS] && o[CPR] * 256.0 >= W && o[NCHUNKS] == (double)N * H * o[CPR]);
            CHECK(o[LDS] <= 160.0 * 1024 && (op == LOSS_UP_METRICS || o[LDS] <= (double)LOSS_LDS_DEFAULT));
        }
        ++n;
    }

    // the multi-operand criteria: 1 .. KD_MULTI_MAX operands, one of them in another layout
    for (int smean = 0; smean < 2; ++smean) for (int nt : {1, 3, KD_MULTI_MAX}) for (int N : {1, 2}) for (int C : {4, 19, 21, 22, 256, 257, 1024, 1025})
    for (long long P : {1LL, 16383LL, 16384LL}) for (int lay = 0; lay < NLAY; ++lay) for (int odd = -1; odd < nt; odd += nt) for (int dt = 0; dt < 2; ++dt)
    for (int off : offs) for (int hg = 0; hg < 2; ++hg) {
        long long s[5], g[5], ts[5 * KD_MULTI_MAX];
        make(s, lay, dt, 0, N, C, P); make(g, lay, smean ? 0 : dt, 0, N, C, P);
        for (int k = 0; k < nt; ++k) make(ts + 5 * k, k == odd ? NCHW : lay, dt, k == nt - 1 ? off : 0, N, C, P);
        if (smean && !hg) continue;     // the mean softmax always has its output
        ls_multi(smean ? nullptr : s, ts, nt, hg ? g : nullptr, smean, N, C, P, o);
        const int k = (int)o[KERNEL];
        const long long rows = (long long)N * P;
        CHECK(o[BLOCKS] >= 1 && o[BLOCKS] <= LOSS_MT_MAX_BLOCKS);
        if (k == LK_KLDM_NHWC) CHECK(!smean && C < 22 && rows >= 16384 && (lay == CL || (lay == BSLICE && N == 1)) && odd < 0 && o[LDS] == 3.0 * 256 * C * 4 && o[LDS] <= (double)LOSS_LDS_DEFAULT);
        else if (k == LK_KLDM || k == LK_KLDM_SMEAN) CHECK((k == LK_KLDM_SMEAN) == (smean != 0) && o[LDS] == 0);
        else {
            CHECK(k >= LK_MT_WAVE_1_VEC + 4 * smean && k <= LK_MT_WAVE_4_NOVEC + 4 * smean && ((lay != NCHW && odd < 0) || P == 1) && C <= 1024 && o[LDS] == 0);
            CHECK(((k - LK_MT_WAVE_1_VEC) % 4 >= 2) == (C > 256) && ((k - LK_MT_WAVE_1_VEC) % 2 == 1 || (C % 4 == 0 && off % (dt ? 8 : 16) == 0)));
            CHECK(o[BLOCKS] == LOSS_MT_MAX_BLOCKS || o[BLOCKS] * 4 >= rows);
        }
        ++n;
    }
    for (int dt = 0; dt < 2; ++dt) for (long long e : {1LL, 7LL, 8LL, 9LL, 1LL << 40}) {
        ls_scale(dt, e, o);
        CHECK((int)o[KERNEL] == LK_SCALE_F32 + dt && o[BLOCKS] >= 1 && o[BLOCKS] <= LOSS_MAX_BLOCKS);
        ++n;
    }
    printf("loss_select sweep: %lld calls walked through every selector, no finding\n", n);
    return 0;
}
