// Stand-alone walk of the dropout rule and selection (csrc/dropout_rng.h, csrc/dropout_select.h through wrap.cpp) for a sanitizer
// build: `make sweep` compiles this with -fsanitize=address,undefined and runs it.  The generator's known answers; the keep decision
// at indices, offsets and seeds around and past the 32-bit boundaries (the index up to the largest an int64 holds); the selector over
// both dtypes, channel counts, pixel strides and base offsets up to the largest sizes the argument predicate admits, each answer held
// to totality: a known kernel of the dtype, 16-B accesses exactly when every gate is open, items that cover M * C exactly once and a
// grid of 1 .. DROPOUT_CAP workgroups.
#include <initializer_list>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/dropout_rng.h"
#include "../../knowledge-distillation-by-replacing-cheap-conv_amd/csrc/dropout_select.h"

extern "C" {
void dr_philox(const uint32_t *ctr, const uint32_t *key, uint32_t *out);
int dr_keep(uint64_t seed, uint64_t offset, int64_t idx, uint32_t threshold);
const char *ds_name(int k);
int ds_args_ok(long long x, int ldx, long long y, int ldy, int dtype, long long M, int C);
int ds_vec_ok(int dtype, int C, long long x, int ldx, long long y, int ldy);
void ds_select(int dtype, long long M, int C, long long x, int ldx, long long y, int ldy, double *out);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "sweep_main.cpp:%d: %s\n", __LINE__, #c); abort(); } } while (0)
enum { KERNEL, VEC, ITEMS, GRID, NOUT };

int main()
{
    long long n_calls = 0;
    {
        const uint32_t c0[4] = {0, 0, 0, 0}, k0[2] = {0, 0}, want0[4] = {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u};
        const uint32_t c1[4] = {~0u, ~0u, ~0u, ~0u}, k1[2] = {~0u, ~0u}, want1[4] = {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu};
        uint32_t o[4];
        dr_philox(c0, k0, o);
        CHECK(!memcmp(o, want0, sizeof o));
        dr_philox(c1, k1, o);
        CHECK(!memcmp(o, want1, sizeof o));
    }
    for (uint64_t seed : {0ull, 123ull, 0xffffffffull, 0x100000000ull, 0x8000000000000001ull, ~0ull})
    for (uint64_t offset : {0ull, 1ull, 0xffffffffull, 0x100000000ull, ~0ull})
    for (int64_t idx : {(int64_t)0, (int64_t)3, (int64_t)4, ((int64_t)1 << 34) - 1, (int64_t)1 << 34, ((int64_t)1 << 34) + 5, INT64_MAX}) {
        ++n_calls;
        CHECK(dr_keep(seed, offset, idx, 0) == 1);                       // threshold 0 keeps everything
        const int k = dr_keep(seed, offset, idx, 0x80000000u);
        CHECK(k == 0 || k == 1);
        CHECK(!dr_keep(seed, offset, idx, 0xffffffffu) || k == 1);       // a higher threshold keeps no more
    }
    for (int k = 0; k < DROPOUT_COUNT; ++k) {
        CHECK(ds_name(k) && strlen(ds_name(k)) > 0);
        for (int j = 0; j < k; ++j) CHECK(strcmp(ds_name(j), ds_name(k)) != 0);
    }
    CHECK(!ds_name(DROPOUT_COUNT) && !ds_name(-1));
    const long long base = 0x10000;
    double o[NOUT];
    for (int dtype : {(int)KD_F32, (int)KD_BF16})
    for (int C : {1, 2, 3, 4, 5, 8, 10, 16, 160, 161, 2147483000}) for (int pad : {0, 1, 2, 4, 8, 32})
    for (long long M : {1ll, 2ll, 105ll, 131072ll, 1ll << 28}) for (int xoff : {0, 4, 8, 16}) for (int yoff : {0, 2, 4, 16}) {
        if (C > 2147483647 - 64) continue;      // (a pixel stride past int32 is not a call)
        if ((double)M * C > 9.0e15) continue;   // (ds_select hands the items back as a double)
        const int es = dtype == KD_BF16 ? 2 : 4, v = 16 / es;
        const int ldx = C + pad, ldy = C + 2 * pad;
        const long long x = base + xoff, y = 2 * base + yoff;
        const bool ok = ds_args_ok(x, ldx, y, ldy, dtype, M, C) != 0;
        CHECK(ok == (xoff % es == 0 && yoff % es == 0));
        if (!ok) continue;
        ++n_calls;
        ds_select(dtype, M, C, x, ldx, y, ldy, o);
        const bool vec = C % v == 0 && ldx % v == 0 && ldy % v == 0 && xoff % 16 == 0 && yoff % 16 == 0;
        CHECK(vec == (ds_vec_ok(dtype, C, x, ldx, y, ldy) != 0));
        CHECK((int)o[KERNEL] == (dtype == KD_BF16 ? 2 : 0) + vec && ds_name((int)o[KERNEL]));
        CHECK(o[VEC] == (vec ? v : 1));
        const long long total = M * C, per = vec ? v : DROPOUT_BLOCK, items = (long long)o[ITEMS];
        CHECK(items * per >= total && (items - 1) * per < total);
        CHECK(o[GRID] >= 1 && o[GRID] <= DROPOUT_CAP && (o[GRID] == DROPOUT_CAP || o[GRID] * DROPOUT_TPB >= items));
    }
    CHECK(!ds_args_ok(0, 4, base, 4, KD_F32, 1, 4) && !ds_args_ok(base, 4, 0, 4, KD_F32, 1, 4) && !ds_args_ok(base, 4, base, 4, 2, 1, 4));
    CHECK(!ds_args_ok(base, 3, base, 4, KD_F32, 1, 4) && !ds_args_ok(base, 4, base, 3, KD_F32, 1, 4) && !ds_args_ok(base, 4, base, 4, KD_F32, 0, 4));
    CHECK(!ds_args_ok(base, 4, base, 4, KD_F32, 1, 0) && !ds_args_ok(base, 4, base, 4, KD_F32, INT64_MAX / 4, 4));
    printf("dropout sweep: %lld calls walked through the rule and the selector, no finding\n", n_calls);
    return 0;
}
