// Which kernel the criterion, metric and optimizer-note entry points of losses.hip run for a call, on what grid and with how much
// dynamic LDS: a pure function of the views (strides, dtypes, the pointers' alignment) and the shape.  The launchers check their
// arguments, call the selector of their family, note loss_kernel_name(sel.kernel) and switch over sel.kernel; kd_loss_workspace
// returns loss_workspace_bytes.  No HIP, no getenv and no globals here: a plain host C++ compiler accepts this file, and
// tests/test_loss_select_host.py holds it against the restatement of tests/_loss_dispatch_cases.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/kdcc.h"
#include "resample.h"

// One value per name the launchers note (loss_kernel_name), then LOSS_REFUSED.  The 24 channels-last forms of the two-operand
// criteria are a range: LK_PAIR_NHWC + 8 * kind + 4 * (s is bf16) + 2 * (t is bf16) + (grad is bf16).
enum LossKernel {
    LK_PAIR_NHWC, LK_PAIR_NHWC_LAST = LK_PAIR_NHWC + 23,
    LK_PAIR_KLD, LK_PAIR_JSD, LK_PAIR_EKL,
    LK_MSE_VEC_F32, LK_MSE_VEC_BF16, LK_MSE_STRIDED, LK_WHMSE,
    LK_CE2D_NHWC_F32, LK_CE2D_NHWC_BF16, LK_CE2D, LK_CE2D_GRAD,
    LK_CONFUSION_NHWC_F32, LK_CONFUSION_NHWC_BF16, LK_CONFUSION,
    LK_CE2D_UP_0, LK_CE2D_UP_19, LK_KLDIV_UP_0, LK_KLDIV_UP_19, LK_JSDIV_UP_0, LK_JSDIV_UP_19,      // LK_CE2D_UP_0 + 2 * LossUpOp + (C == 19)
    LK_FOCAL_UP_0, LK_FOCAL_UP_19, LK_METRICS_UP_0, LK_METRICS_UP_19,
    LK_FOCAL, LK_FOCAL_GRAD,
    LK_TOPK_VEC_F32_CFAST, LK_TOPK_VEC_F32_PFAST, LK_TOPK_VEC_BF16_CFAST, LK_TOPK_VEC_BF16_PFAST, LK_TOPK_GRAD, LK_TOPK_NOGRAD,
    LK_MT_WAVE_1_VEC, LK_MT_WAVE_1_NOVEC, LK_MT_WAVE_4_VEC, LK_MT_WAVE_4_NOVEC,                     // LK_MT_WAVE_1_VEC + 4 * smean + 2 * (C > 256) + !vec
    LK_SM_WAVE_1_VEC, LK_SM_WAVE_1_NOVEC, LK_SM_WAVE_4_VEC, LK_SM_WAVE_4_NOVEC,
    LK_KLDM_NHWC, LK_KLDM, LK_KLDM_SMEAN,
    LK_RADAM, LK_RADAM_MULTI, LK_SCALE_F32, LK_SCALE_BF16,
    LOSS_REFUSED,   // not a kernel: the call is outside what the family's kernels take (LossSel::why)
};
static inline const char *loss_kernel_name(int k)
{
#define LOSS_PAIR_NAMES(K) "pair_nhwc_kernel<" K ",f32,f32,f32>", "pair_nhwc_kernel<" K ",f32,f32,bf16>", "pair_nhwc_kernel<" K ",f32,bf16,f32>", \
        "pair_nhwc_kernel<" K ",f32,bf16,bf16>", "pair_nhwc_kernel<" K ",bf16,f32,f32>", "pair_nhwc_kernel<" K ",bf16,f32,bf16>",                  \
        "pair_nhwc_kernel<" K ",bf16,bf16,f32>", "pair_nhwc_kernel<" K ",bf16,bf16,bf16>"
    static const char *const names[] = {
        LOSS_PAIR_NAMES("kld"), LOSS_PAIR_NAMES("jsd"), LOSS_PAIR_NAMES("ekl"),
        "pair_kernel<kld>", "pair_kernel<jsd>", "pair_kernel<ekl>",
        "mse_vec_kernel<f32>", "mse_vec_kernel<bf16>", "mse_strided_kernel", "whmse_kernel",
        "ce2d_nhwc_kernel<f32>", "ce2d_nhwc_kernel<bf16>", "ce2d_kernel", "ce2d_grad_kernel",
        "confusion_nhwc_kernel<f32>", "confusion_nhwc_kernel<bf16>", "confusion_kernel",
        "ce2d_up_kernel<0>", "ce2d_up_kernel<19>", "pair_up_kernel<kld,0>", "pair_up_kernel<kld,19>", "pair_up_kernel<jsd,0>", "pair_up_kernel<jsd,19>",
        "focal_up_kernel<0>", "focal_up_kernel<19>", "logit_metrics_up_kernel<0>", "logit_metrics_up_kernel<19>",
        "focal_kernel", "focal_grad_kernel",
        "topk_grad_vec_kernel<f32,cfast>", "topk_grad_vec_kernel<f32,pfast>", "topk_grad_vec_kernel<bf16,cfast>", "topk_grad_vec_kernel<bf16,pfast>",
        "topk_grad_kernel", "topk_nograd",
        "mt_wave_kernel<1,vec>", "mt_wave_kernel<1,novec>", "mt_wave_kernel<4,vec>", "mt_wave_kernel<4,novec>",
        "mt_wave_kernel<1,vec,smean>", "mt_wave_kernel<1,novec,smean>", "mt_wave_kernel<4,vec,smean>", "mt_wave_kernel<4,novec,smean>",
        "kldm_nhwc_kernel", "kldm_kernel", "kldm_kernel<smean>",
        "radam_kernel", "radam_multi_kernel", "scale_by_device_scalar_kernel<f32>", "scale_by_device_scalar_kernel<bf16>"};
#undef LOSS_PAIR_NAMES
    static_assert(sizeof(names) / sizeof(names[0]) == LOSS_REFUSED, "one name per kernel value");
    return k >= 0 && k < LOSS_REFUSED ? names[k] : nullptr;
}
static_assert(LK_PAIR_KLD == LK_PAIR_NHWC + 24 && LK_MSE_VEC_BF16 == LK_MSE_VEC_F32 + 1 && LK_CE2D_NHWC_BF16 == LK_CE2D_NHWC_F32 + 1 &&
              LK_CONFUSION_NHWC_BF16 == LK_CONFUSION_NHWC_F32 + 1 && LK_METRICS_UP_19 == LK_CE2D_UP_0 + 9 && LK_TOPK_VEC_BF16_PFAST == LK_TOPK_VEC_F32_CFAST + 3 &&
              LK_SM_WAVE_4_NOVEC == LK_MT_WAVE_1_VEC + 7 && LK_SCALE_BF16 == LK_SCALE_F32 + 1 && KD_F32 == 0 && KD_BF16 == 1,
              "the selectors compute the dtype / class-count / vector variants from the order of LossKernel");

// What the kernels' translation unit is built for; losses.hip asserts the ones its kernels bake in.
constexpr int LOSS_MAX_BLOCKS = 2048;                            // grid cap of a one-partial-array reduction: kd_loss_workspace holds 2 * LOSS_MAX_BLOCKS doubles
constexpr int LOSS_FOCAL_MAX_BLOCKS = 2 * LOSS_MAX_BLOCKS / 3;   // three partial arrays inside them (focal_kernel, focal_up_kernel)
constexpr int LOSS_MT_MAX_BLOCKS = 2 * LOSS_MAX_BLOCKS / 3;      // kd / ce / count partials (kd_kldiv_multi)
constexpr int LOSS_MET_MAX_BLOCKS = LOSS_MAX_BLOCKS / 2;         // ce_s / ce_t / count / sq partials (logit_metrics_up_kernel)
constexpr int LOSS_UP_NW = 160;                                  // source columns of the patch a 256-pixel chunk of the _up kernels stages
constexpr int LOSS_TOPK_MAX_C = 4096;                            // topk_select_kernel keeps C doubles in LDS (32 KiB)
constexpr int LOSS_TOPK_MAX_CHUNKS = 64, LOSS_WHMSE_MAX_CHUNKS = 64;
constexpr size_t LOSS_LDS_DEFAULT = 65536;                       // dynamic LDS a launch gets without hipFuncSetAttribute

enum LossWhy { LOSS_WHY_NONE, LOSS_WHY_CLASSES, LOSS_WHY_SPAN, LOSS_WHY_TOPK_MAX_C };   // why LOSS_REFUSED
enum LossPair { LOSS_KLD = 0, LOSS_JSD = 1, LOSS_EKL = 2 };
enum LossUpOp { LOSS_UP_CE2D, LOSS_UP_KLDIV, LOSS_UP_JSDIV, LOSS_UP_FOCAL, LOSS_UP_METRICS };

struct LossSel {
    LossKernel kernel;
    LossWhy why;
    int blocks;             // workgroups (whmse: chunks x channel blocks x N)
    size_t lds;             // dynamic LDS bytes
    float sh, sw, oh, ow;   // _up: source coordinate = output coordinate * s + o (UpGeom)
    int cpr;                // _up: 256-pixel chunks per output row
    long long nchunks;      // _up: chunks in all
    int chunks;             // whmse, topk: pixel chunks of a plane ...
    long long per_chunk;    // ... and the pixels of one
    size_t aux_off;         // whmse: byte offset of the per-sample weight sums in the workspace; topk: of the kernel's own (N, C) mask
};

// ---- layout predicates ----------------------------------------------------------------------------------------------------------
// dense channels-last: the class vector of a pixel is contiguous and the pixels follow each other (one image may sit in a wider batch buffer)
template <typename V> static inline bool loss_nhwc(const V *v, int N, int C, int64_t P)
{
    return v->sC == 1 && v->sP == C && (v->sN == (int64_t)C * P || N == 1);
}
static inline bool loss_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
// a, b and g (may be null) cover exactly N*C*P elements with the same dense strides and dtype, from 16-B aligned bases, in whole octets
static inline bool loss_dense_same(const kd_view3 *a, const kd_view3 *b, const kd_mview3 *g, int N, int C, int64_t P)
{
    const bool dense = (a->sC == 1 && a->sP == C && a->sN == (int64_t)C * P) || (a->sP == 1 && a->sC == P && a->sN == (int64_t)C * P);
    if (!dense) return false;
    if (a->sN != b->sN || a->sC != b->sC || a->sP != b->sP || a->dtype != b->dtype) return false;
    if (g && (g->sN != a->sN || g->sC != a->sC || g->sP != a->sP || g->dtype != a->dtype)) return false;
    if (!loss_aligned16(a->ptr) || !loss_aligned16(b->ptr) || (g && !loss_aligned16(g->ptr))) return false;
    return ((long long)N * C * P) % 8 == 0;
}
// 4-element vector accesses on a class-contiguous row: whole groups of 4 and every row start 4-element aligned
template <typename V> static inline bool loss_row_vec_ok(const V *v, int N, int C, int64_t P)
{
    return (C & 3) == 0 && ((uintptr_t)v->ptr & (v->dtype == KD_BF16 ? 7u : 15u)) == 0 && (P == 1 || (v->sP & 3) == 0) && (N == 1 || (v->sN & 3) == 0);
}

// ---- grids and the workspace ---------------------------------------------------------------------------------------------------
// one thread per item, 256 a workgroup, at most `cap` workgroups (the kernels stride over the rest)
static inline int loss_blocks_for(long long total, int cap = LOSS_MAX_BLOCKS)
{
    const long long b = (total + 255) / 256;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}
static inline LossSel loss_flat(LossKernel k, long long total, int cap = LOSS_MAX_BLOCKS)
{
    LossSel c{};
    c.kernel = k;
    c.blocks = loss_blocks_for(total, cap);
    return c;
}
// bytes of the partial sums (+ counts): up to LOSS_MAX_BLOCKS workgroups, or the weighted hint loss' (pixel chunks x channel blocks x N)
static inline size_t loss_partial_bytes(int N, int C)
{
    const size_t wh_blocks = (size_t)LOSS_WHMSE_MAX_CHUNKS * ((C + 255) / 256) * (size_t)N;
    return 2 * (wh_blocks > (size_t)LOSS_MAX_BLOCKS ? wh_blocks : (size_t)LOSS_MAX_BLOCKS) * sizeof(double);
}
// ... then the weighted hint loss' per-sample weight sums
static inline size_t loss_workspace_bytes(int N, int C, int64_t P)
{
    (void)P;
    return loss_partial_bytes(N, C) + (size_t)N * sizeof(float) + 64;
}

// ---- kd_kldiv / kd_jsdiv / kd_ensemble_kldiv -----------------------------------------------------------------------------------
// The channels-last kernel stages 2 x 256 x C floats in dynamic LDS; larger class counts -- e.g. the 100-class CIFAR heads -- and
// every other layout take the strided kernel.
static inline LossSel loss_select_pair(LossPair kind, const kd_view3 *s, const kd_view3 *t, const kd_mview3 *grad, int N, int C, int64_t P)
{
    LossSel c = loss_flat((LossKernel)(LK_PAIR_KLD + kind), (long long)N * P);
    const size_t lds = (size_t)2 * 256 * C * sizeof(float);
    if (lds <= LOSS_LDS_DEFAULT && loss_nhwc(s, N, C, P) && loss_nhwc(t, N, C, P) && (!grad || loss_nhwc(grad, N, C, P))) {
        const int gdt = grad ? grad->dtype : s->dtype;
        c.kernel = (LossKernel)(LK_PAIR_NHWC + 8 * kind + 4 * (s->dtype == KD_BF16) + 2 * (t->dtype == KD_BF16) + (gdt == KD_BF16));
        c.lds = lds;
    }
    return c;
}

// ---- kd_hint_mse / kd_weighted_hint_mse ------------------------------------------------------------------------------------------
static inline LossSel loss_select_mse(const kd_view3 *s, const kd_view3 *t, const kd_mview3 *grad, int N, int C, int64_t P)
{
    const long long numel = (long long)N * C * P;
    if (loss_dense_same(s, t, grad, N, C, P)) return loss_flat((LossKernel)(LK_MSE_VEC_F32 + (s->dtype == KD_BF16)), numel / 8);   // an octet per thread and step
    return loss_flat(LK_MSE_STRIDED, numel);
}
// grid (pixel chunks, channel blocks of 256, N): at most 64 chunks of a plane; the partials of all workgroups, then the weight sums
static inline LossSel loss_select_whmse(int N, int C, int64_t P)
{
    LossSel c{};
    c.kernel = LK_WHMSE;
    c.chunks = (int)(P < LOSS_WHMSE_MAX_CHUNKS ? P : LOSS_WHMSE_MAX_CHUNKS);
    c.per_chunk = c.chunks > 0 ? (P + c.chunks - 1) / c.chunks : 0;
    c.blocks = c.chunks * ((C + 255) / 256) * N;
    c.aux_off = loss_partial_bytes(N, C);
    return c;
}

// ---- kd_ce2d / kd_ce2d_weighted / kd_confusion -----------------------------------------------------------------------------------
static inline LossSel loss_select_ce2d(const kd_view3 *x, int N, int C, int64_t P)
{
    LossSel c = loss_flat(LK_CE2D, (long long)N * P);
    const size_t lds = (size_t)256 * C * sizeof(float);     // a class vector per thread
    if (lds <= LOSS_LDS_DEFAULT && loss_nhwc(x, N, C, P)) {
        c.kernel = (LossKernel)(LK_CE2D_NHWC_F32 + (x->dtype == KD_BF16));
        c.lds = lds;
    }
    return c;
}
static inline LossSel loss_select_confusion(const kd_view3 *x, int N, int C, int64_t P)
{
    LossSel c = loss_flat(LK_CONFUSION, (long long)N * P);
    const size_t hist = (size_t)C * C * sizeof(unsigned int), lds = (size_t)256 * C * sizeof(float) + hist;   // fits up to 53 classes
    c.lds = hist;
    if (lds <= LOSS_LDS_DEFAULT && loss_nhwc(x, N, C, P)) {
        c.kernel = (LossKernel)(LK_CONFUSION_NHWC_F32 + (x->dtype == KD_BF16));
        c.lds = lds;
    }
    return c;
}

// ---- kd_ce2d_up / kd_kldiv_up / kd_jsdiv_up / kd_focal_up / kd_logit_metrics_up ------------------------------------------------------
// What differs between the five: how many classes their staged patches take (one patch of 2 x LOSS_UP_NW x C floats, or the
// student's and the teacher's; the metrics kernel reserves its LDS beyond the default limit), how many partials their finishing
// kernel's layout holds, and the metrics kernel's two C x C histograms.
static inline int loss_up_max_classes(LossUpOp op) { return op == LOSS_UP_KLDIV || op == LOSS_UP_JSDIV ? 24 : 48; }
static inline int loss_up_max_blocks(LossUpOp op) { return op == LOSS_UP_FOCAL ? LOSS_FOCAL_MAX_BLOCKS : op == LOSS_UP_METRICS ? LOSS_MET_MAX_BLOCKS : LOSS_MAX_BLOCKS; }
// Total: a class count above the bound or a non-positive extent gives LOSS_REFUSED without touching the geometry's arithmetic
// (the entry points report the latter themselves).
static inline LossSel loss_select_up(LossUpOp op, int N, int h, int w, int C, int H, int W, int align_corners)
{
    LossSel c{};
    c.kernel = LOSS_REFUSED;
    if (C > loss_up_max_classes(op)) { c.why = LOSS_WHY_CLASSES; return c; }
    if (N < 1 || h < 1 || w < 1 || C < 1 || H < 1 || W < 1) return c;
    const ResampleGeom g = resample_geom(h, w, H, W, align_corners);
    c.sh = g.sh; c.sw = g.sw; c.oh = g.oh; c.ow = g.ow;
    // source columns one 256-pixel chunk can touch, (int)(255 * sw) + 3, must fit the staged patch (compared before the
    // conversion: a ratio in the billions has no int)
    if (!(255.f * c.sw < (float)(LOSS_UP_NW - 2))) { c.why = LOSS_WHY_SPAN; return c; }
    c.cpr = (W + 255) / 256;
    c.nchunks = (long long)N * H * c.cpr;
    const int cap = loss_up_max_blocks(op);
    c.blocks = (int)(c.nchunks < cap ? c.nchunks : cap);
    const bool two = op != LOSS_UP_CE2D && op != LOSS_UP_FOCAL;
    c.lds = (size_t)(two ? 4 : 2) * LOSS_UP_NW * C * sizeof(float) + (op == LOSS_UP_METRICS ? (size_t)2 * C * C * sizeof(unsigned int) : 0);
    c.kernel = (LossKernel)(LK_CE2D_UP_0 + 2 * op + (C == 19));     // 19 classes (Cityscapes): the class count at compile time
    return c;
}

// ---- kd_topk_hint_mse ----------------------------------------------------------------------------------------------------------
// pixel chunks of topk_sums_kernel's grid (chunks, channel groups of 64, N): about 2048 workgroups, at most 64 chunks of a plane
static inline int loss_topk_chunks(int N, int C, int64_t P)
{
    const long long groups = (long long)N * ((C + 63) / 64);
    long long ch = 2048 / (groups > 0 ? groups : 1);
    ch = ch < 1 ? 1 : (ch > LOSS_TOPK_MAX_CHUNKS ? LOSS_TOPK_MAX_CHUNKS : ch);
    return (int)(ch > P ? P : ch);
}
// workspace: [t^2 sums | (s-t)^2 sums] x (N*C*chunks) doubles, N per-sample sums, then the mask (16-B aligned: the dense gradient reads it as float4)
static inline size_t loss_topk_mask_off(int N, int C, int chunks) { return (2 * (size_t)N * C * chunks + N + (N & 1)) * sizeof(double); }
static inline size_t loss_topk_workspace_bytes(int N, int C, int64_t P)
{
    if (N <= 0 || C <= 0 || P <= 0) return 64;
    const size_t nc = (size_t)N * C;
    return 2 * nc * loss_topk_chunks(N, C, P) * sizeof(double) + (size_t)N * sizeof(double) + nc * sizeof(float) + 64;
}
// The gradient's kernel (the sums and the selection run for every call).  mask: the caller's (N, C) mask or null, then the
// kernel writes its own into the workspace.
static inline LossSel loss_select_topk(const kd_view3 *s, const kd_view3 *t, const kd_mview3 *grad, const float *mask, const void *workspace,
                                       int N, int C, int64_t P)
{
    LossSel c{};
    c.kernel = LOSS_REFUSED;
    if (C > LOSS_TOPK_MAX_C) { c.why = LOSS_WHY_TOPK_MAX_C; return c; }
    c.chunks = loss_topk_chunks(N, C, P);
    c.per_chunk = c.chunks > 0 ? (P + c.chunks - 1) / c.chunks : 0;
    c.aux_off = loss_topk_mask_off(N, C, c.chunks);
    c.kernel = LK_TOPK_NOGRAD;
    if (!grad) return c;
    const long long numel = (long long)N * C * P;
    const bool cfast = s->sC == 1 && s->sP == C;
    const uintptr_t mk = mask ? (uintptr_t)mask : (uintptr_t)workspace + c.aux_off;
    if (loss_dense_same(s, t, grad, N, C, P) && (cfast ? C % 8 == 0 : P % 8 == 0) && (mk & 15u) == 0) {
        c.kernel = (LossKernel)(LK_TOPK_VEC_F32_CFAST + 2 * (s->dtype == KD_BF16) + !cfast);
        c.blocks = loss_blocks_for(numel / 8);
    } else {
        c.kernel = LK_TOPK_GRAD;
        c.blocks = loss_blocks_for(numel);
    }
    return c;
}

// ---- kd_kldiv_multi / kd_softmax_mean -------------------------------------------------------------------------------------------
// s: the student (null for kd_softmax_mean), ts: 1 .. KD_MULTI_MAX operands (the entry points have checked), g: the gradient (may
// be null) or kd_softmax_mean's output.  A wave per row while the classes are contiguous and at most 1024; few classes and many
// rows would idle most of a wave's lanes: a thread per row then, staged through LDS where everything is dense channels-last
// (the mean softmax has no such kernel).
static inline LossSel loss_select_multi(const kd_view3 *s, const kd_multi_targets *ts, const kd_mview3 *g, bool smean, int N, int C, int64_t P)
{
    bool unit = (!s || s->sC == 1) && (!g || g->sC == 1);
    bool dense = !smean && (!s || loss_nhwc(s, N, C, P)) && (!g || loss_nhwc(g, N, C, P));
    bool vec = (!s || loss_row_vec_ok(s, N, C, P)) && (!g || loss_row_vec_ok(g, N, C, P));
    for (int k = 0; k < ts->n; ++k) {
        unit = unit && ts->t[k].sC == 1;
        dense = dense && loss_nhwc(&ts->t[k], N, C, P);
        vec = vec && loss_row_vec_ok(&ts->t[k], N, C, P);
    }
    const long long rows = (long long)N * P;
    const bool narrow = C < 22 && rows >= 16384;
    LossSel c = loss_flat(smean ? LK_KLDM_SMEAN : LK_KLDM, rows, LOSS_MT_MAX_BLOCKS);
    if (narrow && dense) {
        c.kernel = LK_KLDM_NHWC;
        c.lds = (size_t)3 * 256 * C * sizeof(float);
    } else if (unit && C <= 1024 && !narrow) {
        c.kernel = (LossKernel)(LK_MT_WAVE_1_VEC + 4 * smean + 2 * (C > 256) + !vec);
        c.blocks = (int)((rows + 3) / 4 < LOSS_MT_MAX_BLOCKS ? (rows + 3) / 4 : LOSS_MT_MAX_BLOCKS);      // four rows a workgroup
    }
    return c;
}

// ---- kd_scale_by_device_scalar ---------------------------------------------------------------------------------------------------
static inline LossSel loss_select_scale(int dtype, int64_t n) { return loss_flat((LossKernel)(LK_SCALE_F32 + (dtype == KD_BF16)), n / 8); }
