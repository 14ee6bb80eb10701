// Stand-alone walk of the resampling rule (csrc/resample.h through wrap.cpp) for a sanitizer build: `make sweep` compiles this with
// -fsanitize=address,undefined and runs it.  Every (I, O) of 1..40 x 1..40 and four large pairs in both conventions, through
// buffers of exactly the lengths the entry points fill: the indices inside the axis, the fraction inside [0, 1), every output a
// source index weighs inside its candidate range, the range inside the outputs and no longer than 2/s + 6.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/resample.h"

extern "C" {
void rs_geom(int h, int w, int H, int W, int align_corners, float *out);
void rs_src(int I, int O, float s, float off, int *i0, int *i1, float *f);
void rs_range(int I, int O, float s, float off, int *lo, int *hi);
void rs_weight(int I, int O, float s, float off, float *w);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "sweep_main.cpp:%d: %s (I %d O %d ac %d)\n", __LINE__, #c, I, O, ac); abort(); } } while (0)

static long long n_axes = 0;
static void axis(int I, int O, int ac)
{
    float g[4];
    rs_geom(I, I, O, O, ac, g);
    const float s = g[0], off = g[2];
    CHECK(g[1] == s && g[3] == off && s >= 0.f && off >= -0.5f && (ac ? off == 0.f : s > 0.f));
    std::vector<int> i0(O), i1(O), lo(I), hi(I);
    std::vector<float> f(O), w((size_t)O * I);
    rs_src(I, O, s, off, i0.data(), i1.data(), f.data());
    rs_range(I, O, s, off, lo.data(), hi.data());
    rs_weight(I, O, s, off, w.data());
    for (int o = 0; o < O; ++o) CHECK(0 <= i0[o] && i0[o] <= i1[o] && i1[o] <= I - 1 && i1[o] - i0[o] <= 1 && f[o] >= 0.f && f[o] < 1.f);
    for (int i = 0; i < I; ++i) {
        CHECK(0 <= lo[i] && hi[i] <= O - 1);
        if (s > 0.f) CHECK((float)(hi[i] - lo[i]) <= 2.f / s + 6.f);
        for (int o = 0; o < O; ++o)
            if (w[(size_t)o * I + i] != 0.f) CHECK(lo[i] <= o && o <= hi[i]);
    }
    ++n_axes;
}

int main()
{
    for (int ac = 0; ac < 2; ++ac) {
        for (int I = 1; I <= 40; ++I) for (int O = 1; O <= 40; ++O) axis(I, O, ac);
        axis(33, 1025, ac); axis(128, 1024, ac); axis(256, 2048, ac); axis(1025, 33, ac);
    }
    printf("resample sweep: %lld axes walked, no finding\n", n_axes);
    return 0;
}
