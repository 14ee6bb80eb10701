// Which kernel the classifier-head entry points (head_ops.hip: kd_head_bn_relu_pool_fwd / _bwd) run for a call, and on what grid: a
// pure function of the channel count, the pixel strides and the pointer values of x and dx.  The launcher checks its arguments, calls
// head_select(), notes head_kernel_name(sel.kernel) and launches what sel says.  No HIP, no getenv and no globals here: a plain host
// C++ compiler accepts this file, and tests/test_head_select_host.py holds it to both sides of every gate.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/kdcc.h"

// One value per name the launcher notes: pass (forward, backward) x accesses (scalar, 16 B), then HEAD_COUNT.
enum HeadKernel { HK_FWD_1, HK_FWD_V, HK_BWD_1, HK_BWD_V, HEAD_COUNT };
static inline const char *head_kernel_name(int k)
{
    static const char *const names[] = {"head_fwd_kernel<1>", "head_fwd_kernel<4>", "head_bwd_kernel<1>", "head_bwd_kernel<4>"};
    static_assert(sizeof(names) / sizeof(names[0]) == HEAD_COUNT, "one name per kernel value");
    return k >= 0 && k < HEAD_COUNT ? names[k] : nullptr;
}

// What head_ops.hip is built for; it aliases these or static_asserts against them.
constexpr int HEAD_TPB = 1024;       // threads of every workgroup: 16 waves, to hide the latency of its strided walk over the pixels
constexpr int HEAD_GROUP = 4;        // channels a workgroup owns, over all N * HW pixels: 16 B of fp32, one 16-B access per pixel
constexpr int HEAD_VEC_BYTES = 16;

struct HeadSel {
    HeadKernel kernel;
    int vec;                // channels a thread loads (and stores) at once: 1 or 4
    unsigned grid;          // workgroups of HEAD_TPB = groups of HEAD_GROUP channels
};

// ---- predicates -----------------------------------------------------------------------------------------------------------------
static inline bool head_aligned16(const void *p) { return ((uintptr_t)p & (HEAD_VEC_BYTES - 1)) == 0; }
// N, HW, C >= 1 and a pixel stride that holds the channels
static inline bool head_shape_ok(int32_t N, int32_t HW, int32_t C, int32_t ld) { return N >= 1 && HW >= 1 && C >= 1 && ld >= C; }
// 16-B accesses need every pixel's channel group to start on a 16-B boundary: whole groups, strides of whole groups, aligned bases.
// dx == NULL (the forward; a backward that wants no dx) puts no condition on lddx.
static inline bool head_vec_ok(int32_t C, const void *x, int32_t ldx, const void *dx, int32_t lddx)
{
    return C % HEAD_GROUP == 0 && ldx % HEAD_GROUP == 0 && head_aligned16(x) && (dx == nullptr || (lddx % HEAD_GROUP == 0 && head_aligned16(dx)));
}

// ---- the entry points -----------------------------------------------------------------------------------------------------------
static inline HeadSel head_select(bool backward, int32_t C, const void *x, int32_t ldx, const void *dx, int32_t lddx)
{
    HeadSel s{};
    const bool vec = head_vec_ok(C, x, ldx, backward ? dx : nullptr, lddx);
    s.vec = vec ? HEAD_GROUP : 1;
    s.kernel = (HeadKernel)((backward ? 2 : 0) + (vec ? 1 : 0));
    s.grid = (unsigned)(((long long)C + HEAD_GROUP - 1) / HEAD_GROUP);
    return s;
}
