// Which kernel each Cityscapes batch entry point (seg_data_ops.hip: kd_seg_crop, kd_seg_jitter, kd_seg_finish) runs for a call, and
// on what grid: a pure function of the shapes, the output's dtype, layout, pixel stride and the pointer values.  The launchers check
// their arguments, call the selector, note seg_kernel_name(sel.kernel) and launch what sel says.  No HIP, no getenv and no globals
// here: a plain host C++ compiler accepts this file, and tests/test_seg_data_select_host.py holds it to both sides of every gate.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/kdcc.h"

// One value per name the launchers note.  The sixteen finish kernels are dtype (fp32, bf16) x layout (NCHW, NHWC) x source (gather
// straight from bytes, Gaussian blur through LDS) x stores (scalar, 16 B), in that order of significance.
enum SegKernel {
    SK_CROP_1, SK_CROP_16, SK_JITTER_1, SK_JITTER_16, SK_FINISH_0,
    SEG_COUNT = SK_FINISH_0 + 16,
};
static inline const char *seg_kernel_name(int k)
{
    static const char *const names[] = {
        "seg_crop_kernel<1>", "seg_crop_kernel<16>", "seg_jitter_kernel<1>", "seg_jitter_kernel<16>",
        "seg_finish_kernel<f32,nchw,gather,1>", "seg_finish_kernel<f32,nchw,gather,4>", "seg_finish_kernel<f32,nchw,blur,1>",
        "seg_finish_kernel<f32,nchw,blur,4>", "seg_finish_kernel<f32,nhwc,gather,1>", "seg_finish_kernel<f32,nhwc,gather,4>",
        "seg_finish_kernel<f32,nhwc,blur,1>", "seg_finish_kernel<f32,nhwc,blur,4>", "seg_finish_kernel<bf16,nchw,gather,1>",
        "seg_finish_kernel<bf16,nchw,gather,8>", "seg_finish_kernel<bf16,nchw,blur,1>", "seg_finish_kernel<bf16,nchw,blur,8>",
        "seg_finish_kernel<bf16,nhwc,gather,1>", "seg_finish_kernel<bf16,nhwc,gather,8>", "seg_finish_kernel<bf16,nhwc,blur,1>",
        "seg_finish_kernel<bf16,nhwc,blur,8>"};
    static_assert(sizeof(names) / sizeof(names[0]) == SEG_COUNT, "one name per kernel value");
    return k >= 0 && k < SEG_COUNT ? names[k] : nullptr;
}

// What seg_data_ops.hip is built for; it aliases these or static_asserts against them.
constexpr int SEG_TPB = 256;            // threads of every workgroup
constexpr int SEG_TX = 32, SEG_TY = 16; // an output tile of the crop and finish kernels: SEG_TY rows of SEG_TX pixels
constexpr int SEG_CH = 3;
constexpr int SEG_HDR = 32;             // int32 words of a parameter row's header (data_loader/seg_tables.py documents them)
constexpr int SEG_TAPS = 9;             // the widest resampling window: bicubic support 2 widened by a down-scale of 2
constexpr int SEG_ENTRY = 2 + SEG_TAPS; // [xmin, taps, k0..k8] per output column / row
constexpr int SEG_CAP_C = 2 * SEG_TX + 10, SEG_CAP_R = 2 * SEG_TY + 10;  // source columns / rows a tile's windows may span
constexpr int SEG_MAX_RADIUS = 5;       // int(4 sigma + 0.5), sigma <= 1.3
constexpr int SEG_JITTER_PIXELS = 16;   // pixels a thread of the 16-B jitter kernel owns: 48 bytes, three 16-B accesses
constexpr int SEG_VEC_BYTES = 16;
constexpr int SEG_MAX_SIDE = 1 << 15;   // H, W and S at most
constexpr int SEG_MAX_BATCH = 65535;    // the grid's z

struct SegCropSel {
    SegKernel kernel;
    int store;              // bytes a thread stores at once: 1 or 16
    unsigned gx, gy, gz;    // tiles across, tiles down, samples
};
struct SegJitterSel {
    SegKernel kernel;
    int pixels;             // pixels a thread owns: 1 or SEG_JITTER_PIXELS
    long long chunks;       // threads with work per sample = S * S / pixels
    unsigned gx, gy;        // workgroups per sample, samples
};
struct SegFinishSel {
    SegKernel kernel;
    int vec;                // elements a thread stores at once: 1, or 16 B of the dtype (4 fp32 / 8 bf16)
    int src_vec;            // the gather reads the tile's rows of bytes with 16-B loads
    unsigned gx, gy, gz;
};

// ---- predicates -----------------------------------------------------------------------------------------------------------------
static inline bool seg_dtype_ok(int dtype) { return dtype == KD_F32 || dtype == KD_BF16; }
static inline bool seg_layout_ok(int layout) { return layout == KD_SEG_NCHW || layout == KD_SEG_NHWC; }
static inline int seg_elem_size(int dtype) { return dtype == KD_BF16 ? 2 : 4; }
static inline bool seg_aligned16(const void *p) { return ((uintptr_t)p & (SEG_VEC_BYTES - 1)) == 0; }
static inline bool seg_side_ok(int32_t v) { return v >= 1 && v <= SEG_MAX_SIDE; }
static inline bool seg_batch_ok(int32_t B) { return B >= 1 && B <= SEG_MAX_BATCH; }
// int32 words of a row of the crop's parameter table
static inline long long seg_row_words(int32_t S) { return SEG_HDR + (long long)S * (2 * SEG_ENTRY + 2); }
static inline unsigned seg_tiles(int32_t extent, int tile) { return (unsigned)((extent + tile - 1) / tile); }
static inline size_t seg_jitter_workspace(int32_t B) { return B >= 1 ? (size_t)B * sizeof(uint64_t) : 0; }

// ---- the entry points -----------------------------------------------------------------------------------------------------------
// kd_seg_crop.  16-B stores when both outputs are 16-B aligned and S is a multiple of 16: a tile is then 16 or 32 pixels wide and
// starts, flipped or not, at a multiple of 16 pixels, so every row of its 3-byte pixels and of its mask bytes is whole 16-B pieces.
static inline SegCropSel seg_crop_select(const void *img_out, const void *mask_out, int32_t B, int32_t S)
{
    SegCropSel s{};
    const bool vec = seg_aligned16(img_out) && seg_aligned16(mask_out) && S % 16 == 0;
    s.kernel = vec ? SK_CROP_16 : SK_CROP_1;
    s.store = vec ? 16 : 1;
    s.gx = seg_tiles(S, SEG_TX), s.gy = seg_tiles(S, SEG_TY), s.gz = (unsigned)B;
    return s;
}

// kd_seg_jitter.  A thread owns 16 consecutive pixels (three 16-B accesses) when the image is 16-B aligned and a sample's S * S
// pixels are a multiple of 16 (every sample then starts aligned too); one pixel otherwise.
static inline SegJitterSel seg_jitter_select(const void *img, int32_t B, int32_t S)
{
    SegJitterSel s{};
    const long long pixels = (long long)S * S;
    const bool vec = seg_aligned16(img) && pixels % SEG_JITTER_PIXELS == 0;
    s.kernel = vec ? SK_JITTER_16 : SK_JITTER_1;
    s.pixels = vec ? SEG_JITTER_PIXELS : 1;
    s.chunks = pixels / s.pixels;
    s.gx = (unsigned)((s.chunks + SEG_TPB - 1) / SEG_TPB), s.gy = (unsigned)B;
    return s;
}

// kd_seg_finish.  16-B stores when the image and mask outputs are 16-B aligned and every tile row is whole pieces: NCHW rows of W
// elements, NHWC rows of W * ld elements (a tile starts at a multiple of 32 pixels), and W even for the two-label pieces of the
// int64 mask.  The gather reads with 16-B loads when both sources are 16-B aligned and W is a multiple of 32 (a tile row is then 96
// aligned bytes); the blur stages its halo byte by byte.
static inline SegFinishSel seg_finish_select(int dtype, int layout, int blur, const void *img, const void *mask, const void *out, const void *mask_out,
                                             int32_t B, int32_t H, int32_t W, int32_t ld)
{
    SegFinishSel s{};
    const int v = SEG_VEC_BYTES / seg_elem_size(dtype);
    const long long row = layout == KD_SEG_NHWC ? (long long)W * ld : (long long)W;
    const bool vec = seg_aligned16(out) && seg_aligned16(mask_out) && row % v == 0 && W % 2 == 0;
    s.vec = vec ? v : 1;
    s.src_vec = !blur && seg_aligned16(img) && seg_aligned16(mask) && W % SEG_TX == 0;
    s.kernel = (SegKernel)(SK_FINISH_0 + (dtype == KD_BF16 ? 8 : 0) + (layout == KD_SEG_NHWC ? 4 : 0) + (blur ? 2 : 0) + (vec ? 1 : 0));
    s.gx = seg_tiles(W, SEG_TX), s.gy = seg_tiles(H, SEG_TY), s.gz = (unsigned)B;
    return s;
}
