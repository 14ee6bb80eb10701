// C entry points over csrc/conv_select.h for tests/test_conv_select_host.py (ctypes) and sweep_main.cpp: the selection with
// default switches, its result flattened to ints, and the name the launcher notes for each kernel value.
#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/conv_select.h"

extern "C" {
const char *cs_conv_name(int k)
{
    static const char *const names[] = {
        "conv_row_duo_kernel", "conv_row_persist_kernel<dbg>", "conv_row_lw_kernel", "conv_row_persist_kernel<pp>", "conv_row_persist_kernel<lockstep>",
        "conv_pw_lw_kernel", "conv_igemm_persist_kernel<pp,dual>", "conv_igemm_persist_kernel<pp>", "conv_igemm_persist_kernel<lockstep>",
        "conv_igemm_row_kernel<half>", "conv_row_tall_kernel", "conv_row_pp128_kernel",
        "conv_igemm_row_kernel<narrow>", "conv_igemm_row_kernel<f32,x>", "conv_igemm_row_kernel<x>", "conv_igemm_row_kernel<f32,wide>", "conv_igemm_row_kernel<wide>",
        "conv_igemm_kernel<half>", "conv_igemm_kernel<wide>", "conv_igemm_kernel<deep>", "conv_igemm_kernel<narrow>", "conv_igemm_kernel<narrow2>",
        "conv_igemm_kernel<f32,wide>", "conv_igemm_kernel<f32,deep>", "conv_igemm_kernel<f32,narrow>"};
    return k >= 0 && k <= CONV_IGEMM_F32_NARROW ? names[k] : nullptr;
}
const char *cs_wgrad_name(int k)
{
    static const char *const names[] = {"conv_wgrad_lw_kernel", "conv_wgrad_row_kernel", "conv_wgrad_pw_lw_kernel", "conv_wgrad_wide_kernel", "conv_wgrad_wide_kernel",
                                        "pw_wgrad_tr_kernel", "pw_wgrad_kernel<bf16>", "pw_wgrad_kernel<f32>"};
    return k >= 0 && k <= WGRAD_F32 ? names[k] : nullptr;
}

// out: kernel, epi, grid, ntiles, tn_group, sums_rows, cls_ok, dual_ok, wg_per_cu, nops
void cs_conv_select(const kd_conv_desc *d, const kd_conv_epilogue *ep, int cin1, int ncu, int *out)
{
    const ConvSel c = conv_select(d, ep, cin1, ncu, ConvSwitches{});
    const int v[10] = {c.kernel, c.epi, (int)conv_grid(c, conv_persist_cus(0, ncu)), c.ntiles, c.tn_group, c.sums_rows, c.cls_ok, c.dual_ok, c.wg_per_cu, c.nops};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
}

// d: nullptr = kd_pw_wgrad.  out: kernel, tiles, tiles_ci, splits, rps, grid x, y, z; returns the workspace bound in bytes
unsigned long long cs_wgrad_select(int dtype, long long M, int Cin, int Cout, int taps, const kd_conv_desc *d, int *out)
{
    const WgradSel c = wgrad_select(dtype, M, Cin, Cout, taps, d, WgradSwitches{});
    const int v[8] = {c.kernel, c.tiles, c.tiles_ci, c.splits, c.rps, (int)c.grid[0], (int)c.grid[1], (int)c.grid[2]};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return (unsigned long long)wgrad_workspace_splits((int)M, Cin, Cout, taps, d, WgradSwitches{}) * taps * Cout * Cin * sizeof(float);
}
}
