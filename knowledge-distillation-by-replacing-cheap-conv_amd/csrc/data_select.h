// Which kernel the CIFAR batch entry point (data_ops.hip: kd_cifar_batch) runs for a call, and on what grid: a pure function of the
// batch size, the output's dtype, layout, pixel stride and pointer value.  The launcher checks its arguments, calls data_select(),
// notes data_kernel_name(sel.kernel) and launches what sel says.  No HIP, no getenv and no globals here: a plain host C++ compiler
// accepts this file, and tests/test_cifar_loader_host.py holds it to both sides of every gate.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/kdcc.h"

// One value per name the launcher notes: dtype (fp32, bf16) x layout (NCHW, NHWC) x stores (scalar, 16 B), in that order of
// significance, then DATA_COUNT.
enum DataKernel {
    DK_F32_NCHW_1, DK_F32_NCHW_V, DK_F32_NHWC_1, DK_F32_NHWC_V,
    DK_BF16_NCHW_1, DK_BF16_NCHW_V, DK_BF16_NHWC_1, DK_BF16_NHWC_V,
    DATA_COUNT,
};
static inline const char *data_kernel_name(int k)
{
    static const char *const names[] = {"cifar_batch_kernel<f32,nchw,1>", "cifar_batch_kernel<f32,nchw,4>", "cifar_batch_kernel<f32,nhwc,1>",
                                        "cifar_batch_kernel<f32,nhwc,4>", "cifar_batch_kernel<bf16,nchw,1>", "cifar_batch_kernel<bf16,nchw,8>",
                                        "cifar_batch_kernel<bf16,nhwc,1>", "cifar_batch_kernel<bf16,nhwc,8>"};
    static_assert(sizeof(names) / sizeof(names[0]) == DATA_COUNT, "one name per kernel value");
    return k >= 0 && k < DATA_COUNT ? names[k] : nullptr;
}

// What data_ops.hip is built for; it aliases these or static_asserts against them.
constexpr int DATA_TPB = 256;                  // threads of every workgroup: one item (1 element or 16 B of them) a thread
constexpr int DATA_SIDE = 32;                  // a CIFAR image is DATA_SIDE x DATA_SIDE pixels of DATA_CH interleaved bytes
constexpr int DATA_CH = 3;
constexpr int DATA_PIXELS = DATA_SIDE * DATA_SIDE;
constexpr int DATA_PAD = 4;                    // RandomCrop(32, padding=4): offsets dy, dx in [0, 2 * DATA_PAD]
constexpr int DATA_VEC_BYTES = 16;
constexpr long long DATA_MAX_ELEMS = 1LL << 31;  // elements of the output's storage at most (the grid stays far inside its 32 bits)

struct DataSel {
    DataKernel kernel;
    int vec;                // elements a thread stores at once: 1, or 16 B of the dtype (4 fp32 / 8 bf16)
    long long elems;        // elements of the output's storage the call writes (NHWC: every pixel's whole stride, zero tail included)
    long long items;        // threads that have work = elems / vec
    unsigned grid;          // workgroups of DATA_TPB
};

// ---- predicates -----------------------------------------------------------------------------------------------------------------
static inline bool data_dtype_ok(int dtype) { return dtype == KD_F32 || dtype == KD_BF16; }
static inline bool data_layout_ok(int layout) { return layout == KD_CIFAR_NCHW || layout == KD_CIFAR_NHWC; }
static inline int data_elem_size(int dtype) { return dtype == KD_BF16 ? 2 : 4; }
static inline bool data_aligned16(const void *p) { return ((uintptr_t)p & (DATA_VEC_BYTES - 1)) == 0; }
// Elements the call writes.  The NHWC kernel owns every pixel's whole stride (channels [3, ld) are its zeros), so either layout's
// storage is one dense run: B * 3 * 1024 or B * 1024 * ld elements, always a multiple of 16 bytes.
static inline long long data_elems(int layout, int32_t B, int32_t ld)
{
    return (long long)B * DATA_PIXELS * (layout == KD_CIFAR_NHWC ? ld : DATA_CH);
}
// B >= 1, NHWC: ld >= 3, and the storage within DATA_MAX_ELEMS (checked without overflow)
static inline bool data_shape_ok(int layout, int32_t B, int32_t ld)
{
    if (B < 1 || (layout == KD_CIFAR_NHWC && ld < DATA_CH)) return false;
    const long long per_image = (long long)DATA_PIXELS * (layout == KD_CIFAR_NHWC ? ld : DATA_CH);
    return (long long)B <= DATA_MAX_ELEMS / per_image;
}

// ---- the entry point ------------------------------------------------------------------------------------------------------------
// 16-B stores whenever the base pointer is 16-B aligned: the dense run above is then a whole number of aligned 16-B pieces whatever
// ld is (a piece may straddle pixels; the kernel walks its elements).  Any other base takes the scalar kernel.
static inline DataSel data_select(int dtype, int layout, const void *out, int32_t B, int32_t ld)
{
    DataSel s{};
    const bool vec = data_aligned16(out);
    s.vec = vec ? DATA_VEC_BYTES / data_elem_size(dtype) : 1;
    s.kernel = (DataKernel)((dtype == KD_BF16 ? 4 : 0) + (layout == KD_CIFAR_NHWC ? 2 : 0) + (vec ? 1 : 0));
    s.elems = data_elems(layout, B, ld);
    s.items = s.elems / s.vec;
    s.grid = (unsigned)((s.items + DATA_TPB - 1) / DATA_TPB);
    return s;
}
