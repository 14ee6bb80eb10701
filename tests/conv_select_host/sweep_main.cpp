// Stand-alone walk of the selection (csrc/conv_select.h through wrap.cpp) for a sanitizer build: `make sweep` compiles this with
// -fsanitize=address,undefined and runs it.  Shapes on both sides of every gate of the two selections, every way of asking for
// sums / the classifier epilogue / a second A source; each answer of a query is held against the kernel the same call selects.
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/conv_select.h"

extern "C" {
const char *cs_conv_name(int k);
const char *cs_wgrad_name(int k);
void cs_conv_select(const kd_conv_desc *d, const kd_conv_epilogue *ep, int cin1, int ncu, int *out);
unsigned long long cs_wgrad_select(int dtype, long long M, int Cin, int Cout, int taps, const kd_conv_desc *d, int *out);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "sweep_main.cpp:%d: %s\n", __LINE__, #c); abort(); } } while (0)

static int conv_out(int h, int k, int s, int p, int d) { return (h + 2 * p - d * (k - 1) - 1) / s + 1; }

int main()
{
    alignas(16) static char buf[32];
    long long n = 0;
    const int Hs[] = {1, 4, 8, 15, 16, 34, 223, 224}, Ws[] = {64, 72, 256, 264, 512}, Cs[] = {64, 128, 136, 256, 320, 1280, 2048}, dils[] = {1, 8, 16, 17, 32, 33, 64, 65};
    for (int dtype = 0; dtype < 2; ++dtype) for (int H : Hs) for (int W : Ws) for (int Cin : {64, 128, 256}) for (int Cout : Cs) for (int k : {1, 3}) for (int dil : dils)
    for (int stride : {1, 2}) for (int same = 0; same < 2; ++same) {
        if (k == 1 && (dil > 1 || same)) continue;
        const int pad = k == 1 ? 0 : (same ? dil : 1);
        kd_conv_desc d = {dtype, 2, H, W, Cin, conv_out(H, k, stride, pad, dil), conv_out(W, k, stride, pad, dil), Cout, k, k, stride, pad, dil, Cin};
        if (d.Ho <= 0 || d.Wo <= 0) continue;
        const long long M = (long long)d.N * d.Ho * d.Wo;
        for (int ops = 0; ops < 8; ++ops) for (int outs = 0; outs < 4; ++outs) for (int ask = 0; ask < 2; ++ask) for (int mis = 0; mis < 2; ++mis) for (int cin2 : {0, 64})
        for (int ncu : {256, 304, 64}) {
            kd_conv_epilogue ep;
            memset(&ep, 0, sizeof(ep));
            if (ops & 1) { ep.res_pre = buf + 8 * mis; ep.ld_res_pre = Cout; }
            if (ops & 2) { ep.mask = buf; ep.ld_mask = Cout; }
            if (ops & 4) { ep.res_post = buf; ep.ld_res_post = Cout; }
            if (outs & 1) { ep.out_raw = buf; ep.ld_raw = Cout; }
            if (outs & 2) { ep.out_act = buf; ep.ld_act = Cout; }
            const bool cls = !outs;
            if (cls) { ep.cls_w = buf; ep.cls_out = (float *)buf; ep.ld_cls = ep.ncls = 19; }
            ep.bn_sums = ask ? (float *)buf : nullptr;
            kd_conv_desc t = d;
            t.Cin += cin2;
            int o[10], q[10];
            cs_conv_select(&t, &ep, cin2 ? Cin : 0, ncu, o);
            const char *name = cs_conv_name(o[0]);
            CHECK(name);
            ep.bn_sums = nullptr;
            cs_conv_select(&t, &ep, cin2 ? Cin : 0, ncu, q);
            CHECK(q[5] == o[5] && (o[5] == 0 || o[5] == M / 128));   // the sums answer does not depend on having been acted on
            if (ask && o[5] && !cls) CHECK((ep.mask ? o[1] == (o[9] | 4) : o[1] == 8) && (strstr(name, "<pp") || strstr(name, "_lw_") || strstr(name, "tall") || strstr(name, "pp128")));
            if (o[6]) CHECK(!strcmp(name, "conv_row_lw_kernel") && (!cls || o[1] == 16));
            CHECK((o[7] != 0) == !strcmp(name, "conv_igemm_persist_kernel<pp,dual>") && (cin2 || !o[7]));
            CHECK(o[2] > 0 && o[3] > 0 && (o[8] ? o[2] % 8 == 0 && o[2] <= o[3] + 7 : o[2] == o[3]));
            ++n;
        }
        if (stride == 1) {
            int o[8];
            for (int conv = 0; conv < 2; ++conv) {
                if (!conv && (k != 1)) continue;
                const unsigned long long ws = cs_wgrad_select(dtype, M, Cin, Cout, k * k, conv ? &d : nullptr, o);
                CHECK(cs_wgrad_name(o[0]) && o[3] >= 1 && o[4] >= 1 && (long long)o[3] * o[4] >= M && (long long)(o[3] - 1) * o[4] < M);
                CHECK(ws >= (unsigned long long)o[3] * k * k * Cout * Cin * 4);   // the bound covers the plan taken
                ++n;
            }
        }
    }
    printf("conv_select sweep: %lld selections, no finding\n", n);
    return 0;
}
