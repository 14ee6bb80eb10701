// C entry points over csrc/dw_select.h for tests/test_dw_select_host.py (ctypes) and sweep_main.cpp: the selection with default
// switches (or with the lone-wave kernel switched off, as kd_dwconv_fwd_fanout selects again when the item table fails), its result
// flattened to ints, the queries, and the name the launchers note for each kernel value.
#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/dw_select.h"

extern "C" {
const char *ds_name(int k) { return k == DW_EACH ? "each" : dw_kernel_name(k); }

// facts: bit 0 = every pointer 16-B aligned, 1 = bias / epilogue operand, 2 = stream capturing, 3 = KDCC_DW_LW=0
// out: kernel, nb, fan, lp, nty, ntx, nitems, nseg, ncg, lds, slabs, tile_s, tile_r; returns the workgroups
long long ds_select(int op, const kd_dw_desc *d, int n, int lattice, int facts, int ld_dy, int *out)
{
    DwSwitches sw;
    if (facts & 8) sw.lw = 0;
    const DwSel c = dw_select((DwOp)op, d, n, lattice != 0, DwFacts{(facts & 1) != 0, ld_dy, (facts & 2) != 0, (facts & 4) != 0}, sw);
    const int v[13] = {c.kernel, c.nb, c.fan, c.lp, c.nty, c.ntx, c.nitems, c.nseg, c.ncg, c.lds, c.slabs, c.tile_s, c.tile_r};
    for (int i = 0; i < 13; ++i) out[i] = v[i];
    return c.blocks;
}
int ds_chunk(int n, int done) { return dw_chunk(n, done); }
int ds_lattice_ok(const kd_dw_desc *d, int n) { return dw_lattice_ok(d, n, DwSwitches{}); }
long long ds_lattice_rows(int N, int H, int W, int dil) { return dw_lattice_rows(N, H, W, dil); }
unsigned long long ds_wgrad_workspace(const kd_dw_desc *d) { return dw_wgrad_workspace(d, DwSwitches{}); }
unsigned long long ds_wgrad_multi_workspace(const kd_dw_desc *d, int n) { return dw_wgrad_multi_workspace(d, n, DwSwitches{}); }
}
