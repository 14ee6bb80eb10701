// Which kernel kd_dropout_nhwc (dropout.hip) runs for a call, and on what grid: a pure function of the dtype, the sizes, the pixel
// strides and the pointer values of x and y.  The launcher checks its arguments with dropout_args_ok(), calls dropout_select(), notes
// dropout_kernel_name(sel.kernel) and launches what sel says.  No HIP, no getenv and no globals here: a plain host C++ compiler
// accepts this file, and tests/test_dropout_host.py holds it to both sides of every gate.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/kdcc.h"

// One value per name the launcher notes: dtype (fp32, bf16) x accesses (scalar, 16 B), then DROPOUT_COUNT.
enum DropoutKernel { DK_F32_1, DK_F32_V, DK_BF16_1, DK_BF16_V, DROPOUT_COUNT };
static inline const char *dropout_kernel_name(int k)
{
    static const char *const names[] = {"dropout_block_kernel<float>", "dropout_vec_kernel<float, 4>", "dropout_block_kernel<bf16_t>",
                                        "dropout_vec_kernel<bf16_t, 8>"};
    static_assert(sizeof(names) / sizeof(names[0]) == DROPOUT_COUNT, "one name per kernel value");
    return k >= 0 && k < DROPOUT_COUNT ? names[k] : nullptr;
}

// What dropout.hip is built for; it aliases these or static_asserts against them.
constexpr int DROPOUT_TPB = 256;         // threads of every workgroup
constexpr int DROPOUT_CAP = 2048;        // workgroups at most, 8 per CU: the kernels stride over the rest
constexpr int DROPOUT_VEC_BYTES = 16;    // bytes a lane of the vector kernels owns: 4 fp32 (1 Philox block) or 8 bf16 channels (2 blocks)
constexpr int DROPOUT_BLOCK = 4;         // elements of one Philox block: what a lane of the scalar kernels owns

struct DropoutSel {
    DropoutKernel kernel;
    int vec;                // channels a lane loads (and stores) at once: 4 / 8, or 1 in the scalar kernels
    long long items;        // lanes' worth of work: M * (C / vec) pixel-channel groups, or ceil(M * C / 4) Philox blocks
    unsigned grid;          // workgroups of DROPOUT_TPB
};

// ---- predicates -----------------------------------------------------------------------------------------------------------------
static inline int dropout_elem_size(int32_t dtype) { return dtype == KD_BF16 ? 2 : 4; }
static inline bool dropout_aligned(const void *p, int bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }
// a known dtype, non-null operands aligned to their element, M, C >= 1, pixel strides that hold the channels, and offsets
// (M - 1) * ld + C and indices M * C that an int64 holds with room to stride past the end
static inline bool dropout_args_ok(const void *x, int32_t ldx, const void *y, int32_t ldy, int32_t dtype, int64_t M, int32_t C)
{
    if (dtype != KD_F32 && dtype != KD_BF16) return false;
    const int es = dropout_elem_size(dtype);
    if (!x || !y || !dropout_aligned(x, es) || !dropout_aligned(y, es)) return false;
    if (M < 1 || C < 1 || ldx < C || ldy < C) return false;
    return M <= (INT64_MAX >> 2) / (ldx > ldy ? ldx : ldy);
}
// 16-B accesses need every lane's channel group to start on a 16-B boundary in both views: whole groups per pixel, pixel strides of
// whole groups, aligned bases.  (x == y passes or fails as one view.)
static inline bool dropout_vec_ok(int32_t dtype, int32_t C, const void *x, int32_t ldx, const void *y, int32_t ldy)
{
    const int v = DROPOUT_VEC_BYTES / dropout_elem_size(dtype);
    return C % v == 0 && ldx % v == 0 && ldy % v == 0 && dropout_aligned(x, DROPOUT_VEC_BYTES) && dropout_aligned(y, DROPOUT_VEC_BYTES);
}

// ---- the grid and the entry point -------------------------------------------------------------------------------------------------
// one lane per item, DROPOUT_TPB a workgroup, at most DROPOUT_CAP workgroups
static inline unsigned dropout_grid(long long items)
{
    const long long b = (items + DROPOUT_TPB - 1) / DROPOUT_TPB;
    return (unsigned)(b < 1 ? 1 : (b > DROPOUT_CAP ? DROPOUT_CAP : b));
}

static inline DropoutSel dropout_select(int32_t dtype, int64_t M, int32_t C, const void *x, int32_t ldx, const void *y, int32_t ldy)
{
    DropoutSel s{};
    const bool vec = dropout_vec_ok(dtype, C, x, ldx, y, ldy);
    s.vec = vec ? DROPOUT_VEC_BYTES / dropout_elem_size(dtype) : 1;
    s.kernel = (DropoutKernel)((dtype == KD_BF16 ? 2 : 0) + (vec ? 1 : 0));
    s.items = vec ? (long long)M * (C / s.vec) : ((long long)M * C + DROPOUT_BLOCK - 1) / DROPOUT_BLOCK;
    s.grid = dropout_grid(s.items);
    return s;
}
