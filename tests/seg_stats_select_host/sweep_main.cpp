// Stand-alone walk of the class-statistics selection (csrc/seg_stats_select.h through wrap.cpp) for a sanitizer build: `make sweep`
// compiles this with -fsanitize=address,undefined and runs it.  The selector over image counts, sides and tiles up to the largest
// the shape check admits and base offsets; each answer held to a restated selection and to totality: a known kernel, units that
// cover every row of every tile exactly once, a grid of at least one block, and uint32 partials that cannot overflow.  The
// rows-per-workgroup rule is also walked over byte budgets beyond the shipped one, where the overflow bound is the tighter limit.
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/seg_stats_select.h"

extern "C" {
const char *st_name(int k);
int st_rows(int tile, long long budget);
void st_select(long long targets, long long n, int H, int W, int tile, double *out);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "sweep_main.cpp:%d: %s\n", __LINE__, #c); abort(); } } while (0)

int main()
{
    long long n_calls = 0;
    for (int k = 0; k < SEG_STATS_COUNT; ++k) CHECK(st_name(k) && strlen(st_name(k)) > 0);
    CHECK(strcmp(st_name(0), st_name(1)) != 0 && !st_name(SEG_STATS_COUNT) && !st_name(-1));
    const auto tiles = {1, 2, 7, 8, 15, 16, 17, 20, 32, 40, 48, 64, 255, 256, 1000, 1024, 4096, 8192, 16384, 32767, SEG_MAX_SIDE};
    for (int tile : tiles) for (long long budget : {1LL, 4096LL, 1LL << 16, 1LL << 20, 1LL << 24, 1LL << 30, 1LL << 40}) {
        const long long rows = st_rows(tile, budget), t = tile, row_sum = t * (t - 1) / 2;
        CHECK(rows >= 1 && rows <= t && (rows == 1 || rows * t <= budget));
        CHECK(rows * row_sum <= 0xffffffffLL && t * rows * (rows - 1) / 2 <= 0xffffffffLL);     // the uint32 partials hold a unit
        long long want = budget / t;
        if (row_sum > 0 && want > 0xffffffffLL / row_sum) want = 0xffffffffLL / row_sum;
        if (want > t) want = t;
        if (want < 1) want = 1;
        CHECK(rows == want);
        ++n_calls;
    }
    const long long base = 0x10000;
    double o[9];
    for (long long n : {1LL, 2LL, 64LL, 2975LL, 2147483647LL}) for (int H : {1, 40, 300, 1024, 4096, SEG_MAX_SIDE})
    for (int W : {1, 44, 72, 520, 2048, 4096, SEG_MAX_SIDE}) for (int tile : tiles) for (int off : {0, 1, 8, 16}) {
        st_select(base + off, n, H, W, tile, o);
        const bool vec = off % 16 == 0 && W % 16 == 0 && tile % 16 == 0;
        CHECK((int)o[0] == (vec ? SSK_STATS_16 : SSK_STATS_1) && o[2] == (vec ? 16 : 1) && st_name((int)o[0]));
        CHECK(o[3] == H / tile && o[4] == W / tile);
        const long long rows = (long long)o[5], chunks = (long long)o[6];
        CHECK(rows == st_rows(tile, SEG_STATS_WG_BYTES) && chunks == (tile + rows - 1) / rows && (chunks - 1) * rows < tile);
        const double units = (double)n * (H / tile) * (W / tile) * (double)chunks;
        CHECK(o[7] == units && o[1] == (units > 0 ? 1 : 0));
        CHECK(o[8] == (units < SEG_STATS_MAX_GRID ? units : (double)SEG_STATS_MAX_GRID) && (o[8] >= 1 || !o[1]));
        ++n_calls;
    }
    printf("seg_stats_select sweep: %lld calls walked through the selector, no finding\n", n_calls);
    return 0;
}
