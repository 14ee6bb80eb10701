// Stand-alone walk of the depthwise selection (csrc/dw_select.h through wrap.cpp) for a sanitizer build: `make sweep` compiles this
// with -fsanitize=address,undefined and runs it.  Shapes on both sides of every gate, every entry point, every chunk of 1 .. 7
// branches, every combination of the facts; each answer of a query is held against the plan the same call selects.
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/dw_select.h"

extern "C" {
const char *ds_name(int k);
long long ds_select(int op, const kd_dw_desc *d, int n, int lattice, int facts, int ld_dy, int *out);
int ds_chunk(int n, int done);
int ds_lattice_ok(const kd_dw_desc *d, int n);
unsigned long long ds_wgrad_workspace(const kd_dw_desc *d);
unsigned long long ds_wgrad_multi_workspace(const kd_dw_desc *d, int n);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "sweep_main.cpp:%d: %s\n", __LINE__, #c); abort(); } } while (0)
enum { KERNEL, NB, FAN, LP, NTY, NTX, NITEMS, NSEG, NCG, LDS, SLABS, TILE_S, TILE_R, NOUT };

int main()
{
    long long n = 0;
    const int Hs[] = {1, 24, 131, 136, 1024}, Ws[] = {9, 261, 1024}, Cs[] = {8, 16, 24, 4096}, dils[] = {1, 5, 255, 256};
    for (int dtype = 0; dtype < 2; ++dtype) for (int N : {1, 64}) for (int H : Hs) for (int W : Ws) for (int C : Cs) for (int k : {3, 9}) for (int dil : dils)
    for (int pitch : {0, 4, 1024 - 8, 1024}) for (int pitch_y : {0, 4}) {
        if (pitch >= 1000 && pitch < C) continue;
        const int ldx = pitch >= 1000 ? pitch : C + pitch, ldy = C + pitch_y;
        const kd_dw_desc d = {dtype, N, H, W, C, k, dil * (k - 1) / 2, dil, ldx, ldy};
        const unsigned long long slab = (unsigned long long)k * k * C * 4, ws1 = ds_wgrad_workspace(&d);
        for (int facts = 0; facts < 16; ++facts) for (int ld_dy : {C, C + 4, 1024}) {
            int o[NOUT];
            for (int op = DW_FWD; op <= DW_WGRAD_MULTI; ++op) for (int m = 1; m <= 4; ++m) for (int lattice = 0; lattice < 2; ++lattice) {
                const long long blocks = ds_select(op, &d, m, lattice, facts, ld_dy, o);
                const char *name = ds_name(o[KERNEL]);
                CHECK(name);
                const bool each = o[KERNEL] == DW_EACH, reg = o[KERNEL] <= DW_REG_WGRAD_F32;
                CHECK(each == ((op == DW_SUM || op == DW_FANOUT || op == DW_WGRAD_MULTI) && !strstr(name, "mfma") && !strstr(name, "_lw_")));
                if (each) continue;
                CHECK(blocks > 0 && blocks <= 0x7fffffffLL && o[NITEMS] > 0 && o[NSEG] >= 1 && o[NCG] >= 1);
                if (reg) { CHECK(o[LDS] == 0 && m >= 1 && (op == DW_FWD || op == DW_WGRAD)); continue; }
                // the matrix cores: never outside their domain, whatever else the call looks like
                CHECK(dtype == KD_BF16 && k == 9 && C % 16 == 0 && ldx % 8 == 0 && (facts & 1) && !(facts & 2) && (long long)H * W * ldx * 2 < 0x80000000LL);
                CHECK(o[NB] == m && m <= 3 && o[LP] == lattice && (!lattice || (m >= 2 && ds_lattice_ok(&d, m))));
                CHECK(o[LDS] > 0 && o[LDS] <= 160 * 1024 && o[NSEG] <= o[NITEMS] && blocks == (long long)N * o[NCG] * o[NSEG]);
                if (o[KERNEL] == DW_LW_FAN3) CHECK(op == DW_FANOUT && m == 3 && !lattice && !(facts & 12) && ldy % 8 == 0 && o[NTY] <= 255 && o[NTX] <= 255 && dil <= 255);
                if (op == DW_WGRAD || op == DW_WGRAD_MULTI) CHECK(o[SLABS] == N * o[NSEG] && (lattice || (ld_dy % 8 == 0 && (op == DW_WGRAD || ld_dy >= C))));
                else CHECK(o[SLABS] == 0 && ((lattice && op == DW_FANOUT) || ldy % 8 == 0));
            }
            // the bounds against the plan the same call selects: the single gradient, and every chunk of 1 .. 7 branches
            if (facts & 14) continue;   // (of the facts, the weight gradients read the pointers' alignment alone)
            ds_select(DW_WGRAD, &d, 1, 0, facts, ld_dy, o);
            CHECK(o[SLABS] > 0 && ws1 >= o[SLABS] * slab);
            for (int nb = 1; nb <= 7; ++nb) {
                const unsigned long long wsn = ds_wgrad_multi_workspace(&d, nb);
                CHECK(wsn >= ws1);
                for (int done = 0, m; done < nb; done += m) {
                    m = ds_chunk(nb, done);
                    CHECK(m >= 1 && m <= 3 && (m == 3 || done + m == nb));
                    int q[NOUT];
                    ds_select(DW_WGRAD_MULTI, &d, m, 0, facts, ld_dy, q);
                    CHECK(wsn >= (q[KERNEL] == DW_EACH ? o[SLABS] * slab : (unsigned long long)q[SLABS] * m * slab));
                    if (m >= 2) {
                        ds_select(DW_WGRAD_MULTI, &d, m, 1, facts, C, q);
                        CHECK(q[KERNEL] == DW_EACH || wsn >= (unsigned long long)q[SLABS] * m * slab);
                    }
                }
            }
            ++n;
        }
    }
    printf("dw_select sweep: %lld calls walked through every entry point, no finding\n", n);
    return 0;
}
