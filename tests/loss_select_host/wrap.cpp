// C entry points over csrc/loss_select.h for tests/test_loss_select_host.py (ctypes) and sweep_main.cpp: every selector with its
// views flattened -- a view is five 64-bit integers (pointer value, dtype, sN, sC, sP), a null pointer to them an absent operand --
// its result flattened to doubles, the constants, the workspace sizes and the name the launchers note for each kernel value.
#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/loss_select.h"

namespace {
kd_view3 view(const long long *v) { return kd_view3{(const void *)(uintptr_t)v[0], (int32_t)v[1], v[2], v[3], v[4]}; }
kd_mview3 mview(const long long *v) { return kd_mview3{(void *)(uintptr_t)v[0], (int32_t)v[1], v[2], v[3], v[4]}; }
// out: kernel, why, blocks, lds, cpr, nchunks, chunks, per_chunk, aux_off, sh, sw, oh, ow
void flat(const LossSel &c, double *out)
{
    const double v[13] = {(double)c.kernel, (double)c.why, (double)c.blocks, (double)c.lds, (double)c.cpr, (double)c.nchunks, (double)c.chunks,
                          (double)c.per_chunk, (double)c.aux_off, c.sh, c.sw, c.oh, c.ow};
    for (int i = 0; i < 13; ++i) out[i] = v[i];
}
}  // namespace

extern "C" {
const char *ls_name(int k) { return loss_kernel_name(k); }
int ls_refused(void) { return LOSS_REFUSED; }
// MAX_BLOCKS, FOCAL_MAX_BLOCKS, MT_MAX_BLOCKS, MET_MAX_BLOCKS, UP_NW, TOPK_MAX_C, the default LDS limit
long long ls_const(int i)
{
    const long long v[7] = {LOSS_MAX_BLOCKS, LOSS_FOCAL_MAX_BLOCKS, LOSS_MT_MAX_BLOCKS, LOSS_MET_MAX_BLOCKS, LOSS_UP_NW, LOSS_TOPK_MAX_C, (long long)LOSS_LDS_DEFAULT};
    return i >= 0 && i < 7 ? v[i] : -1;
}
int ls_up_max_classes(int op) { return loss_up_max_classes((LossUpOp)op); }
int ls_up_max_blocks(int op) { return loss_up_max_blocks((LossUpOp)op); }
int ls_blocks_for(long long total) { return loss_blocks_for(total); }
unsigned long long ls_workspace(int N, int C, long long P) { return loss_workspace_bytes(N, C, P); }
unsigned long long ls_topk_workspace(int N, int C, long long P) { return loss_topk_workspace_bytes(N, C, P); }

void ls_pair(int kind, const long long *s, const long long *t, const long long *g, int N, int C, long long P, double *out)
{
    const kd_view3 sv = view(s), tv = view(t);
    const kd_mview3 gv = g ? mview(g) : kd_mview3{};
    flat(loss_select_pair((LossPair)kind, &sv, &tv, g ? &gv : nullptr, N, C, P), out);
}
void ls_mse(const long long *s, const long long *t, const long long *g, int N, int C, long long P, double *out)
{
    const kd_view3 sv = view(s), tv = view(t);
    const kd_mview3 gv = g ? mview(g) : kd_mview3{};
    flat(loss_select_mse(&sv, &tv, g ? &gv : nullptr, N, C, P), out);
}
void ls_whmse(int N, int C, long long P, double *out) { flat(loss_select_whmse(N, C, P), out); }
void ls_ce2d(const long long *x, int N, int C, long long P, double *out)
{
    const kd_view3 xv = view(x);
    flat(loss_select_ce2d(&xv, N, C, P), out);
}
void ls_confusion(const long long *x, int N, int C, long long P, double *out)
{
    const kd_view3 xv = view(x);
    flat(loss_select_confusion(&xv, N, C, P), out);
}
void ls_up(int op, int N, int h, int w, int C, int H, int W, int align_corners, double *out)
{
    flat(loss_select_up((LossUpOp)op, N, h, w, C, H, W, align_corners), out);
}
// mask, workspace: pointer values
void ls_topk(const long long *s, const long long *t, const long long *g, long long mask, long long workspace, int N, int C, long long P, double *out)
{
    const kd_view3 sv = view(s), tv = view(t);
    const kd_mview3 gv = g ? mview(g) : kd_mview3{};
    flat(loss_select_topk(&sv, &tv, g ? &gv : nullptr, (const float *)(uintptr_t)mask, (const void *)(uintptr_t)workspace, N, C, P), out);
}
// ts: nt views one after the other, 1 <= nt <= KD_MULTI_MAX (the entry points' own check)
void ls_multi(const long long *s, const long long *ts, int nt, const long long *g, int smean, int N, int C, long long P, double *out)
{
    const kd_view3 sv = s ? view(s) : kd_view3{};
    const kd_mview3 gv = g ? mview(g) : kd_mview3{};
    kd_multi_targets mt{};
    mt.n = nt < 1 ? 1 : (nt > KD_MULTI_MAX ? KD_MULTI_MAX : nt);
    for (int k = 0; k < mt.n; ++k) { mt.t[k] = view(ts + 5 * k); mt.w[k] = 1.f; }
    flat(loss_select_multi(s ? &sv : nullptr, &mt, g ? &gv : nullptr, smean != 0, N, C, P), out);
}
void ls_scale(int dtype, long long n, double *out) { flat(loss_select_scale(dtype, n), out); }
}
