// Which kernel the Gated-SCNN shape-stream entry points (gscnn_ops.hip, gscnn_bwd.hip) run for a call, on what grid, with how many
// threads and how much dynamic LDS, and what they turn down: a pure function of the shape, the dtypes and the operands' pointer
// values and leading dimensions (kd_gated_conv: and of its one A/B switch, handed in as a bool).  The launchers check their
// pointers, call the selector of their entry point, turn a refusal into their own message and code, note gs_kernel_name(sel.kernel)
// and switch over sel.kernel; the two workspace queries return the functions below.  No device code, no environment and no globals
// here: a plain host C++ compiler accepts this file, and tests/test_gscnn_select_host.py holds it against
// tests/_shape_stream_cases.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/kdcc.h"
#include "resample.h"

// One value per name the launchers note (gs_kernel_name), then GS_REFUSED.  Variants are ranges: <f32 before bf16> x <channel
// counts ascending>; the small_linear templates ascending; the pointwise pairs descending, as the stream runs them.
enum GsKernel {
    GS_GATED_F32_8, GS_GATED_F32_16, GS_GATED_F32_32, GS_GATED_BF16_8, GS_GATED_BF16_16, GS_GATED_BF16_32,   // GS_GATED_F32_8 + 3 * bf16 + index of C
    GS_GATED_MFMA_8, GS_GATED_MFMA_16, GS_GATED_MFMA_32,                                                     // GS_GATED_MFMA_8 + index of C
    GS_EDGE_ATTENTION_F32, GS_EDGE_ATTENTION_BF16,
    GS_EDGE_ASPP_F32, GS_EDGE_ASPP_BF16,
    GS_CONV3X3_16, GS_CONV3X3_32, GS_CONV3X3_64,
    GS_POINTWISE_64_32, GS_POINTWISE_32_16, GS_POINTWISE_16_8,
    GS_SMALL_LINEAR_8, GS_SMALL_LINEAR_16, GS_SMALL_LINEAR_24, GS_SMALL_LINEAR_40, GS_SMALL_LINEAR_72,       // GS_SMALL_LINEAR_8 + index of the template
    GS_RANK1_ADD_F32, GS_RANK1_ADD_BF16,
    // the fixed launch sequences, named by their first kernel: partial then finish; one launch; one launch; gradient, NMS, sweeps,
    // finish; sweeps, finish
    GS_SMALL_WGRAD, GS_GATE_MIX_BWD, GS_EDGE_ATTENTION_BWD, GS_CANNY, GS_CANNY_CONTINUE,
    GS_REFUSED,   // not a kernel: the call is outside what the entry point's kernels take (GsSel::why says which check it fails)
};
static inline const char *gs_kernel_name(int k)
{
    static const char *const names[] = {
        "gated_conv_kernel<f32,8>", "gated_conv_kernel<f32,16>", "gated_conv_kernel<f32,32>",
        "gated_conv_kernel<bf16,8>", "gated_conv_kernel<bf16,16>", "gated_conv_kernel<bf16,32>",
        "gated_conv_mfma_kernel<8>", "gated_conv_mfma_kernel<16>", "gated_conv_mfma_kernel<32>",
        "edge_attention_kernel<f32>", "edge_attention_kernel<bf16>",
        "edge_aspp_kernel<f32>", "edge_aspp_kernel<bf16>",
        "conv3x3_small_kernel<16>", "conv3x3_small_kernel<32>", "conv3x3_small_kernel<64>",
        "pointwise_small_kernel<64,32>", "pointwise_small_kernel<32,16>", "pointwise_small_kernel<16,8>",
        "small_linear_kernel<8>", "small_linear_kernel<16>", "small_linear_kernel<24>", "small_linear_kernel<40>", "small_linear_kernel<72>",
        "rank1_add_kernel<f32>", "rank1_add_kernel<bf16>",
        "small_wgrad_partial_kernel", "gate_mix_bwd_kernel", "edge_attention_bwd_kernel", "canny_grad_kernel", "canny_hyst_kernel"};
    static_assert(sizeof(names) / sizeof(names[0]) == GS_REFUSED, "one name per kernel value");
    return k >= 0 && k < GS_REFUSED ? names[k] : nullptr;
}
static_assert(GS_GATED_BF16_8 == GS_GATED_F32_8 + 3 && GS_GATED_BF16_32 == GS_GATED_F32_8 + 5 && GS_GATED_MFMA_32 == GS_GATED_MFMA_8 + 2 &&
              GS_EDGE_ATTENTION_BF16 == GS_EDGE_ATTENTION_F32 + 1 && GS_EDGE_ASPP_BF16 == GS_EDGE_ASPP_F32 + 1 && GS_CONV3X3_64 == GS_CONV3X3_16 + 2 &&
              GS_POINTWISE_16_8 == GS_POINTWISE_64_32 + 2 && GS_SMALL_LINEAR_72 == GS_SMALL_LINEAR_8 + 4 && GS_RANK1_ADD_BF16 == GS_RANK1_ADD_F32 + 1 &&
              KD_F32 == 0 && KD_BF16 == 1,
              "the selectors compute the dtype / channel variants from the order of GsKernel");

// The first check of its entry point a refused call fails, in the order the entry points have always made them.
enum GsWhy {
    GS_WHY_NONE,
    GS_WHY_SHAPE,       // a pixel, image, channel or sweep count out of range
    GS_WHY_DTYPE,       // not fp32 / bf16 (kd_edge_attention_bwd: or fewer than 8 channels a pixel)
    GS_WHY_MASK,        // kd_small_linear: a mask narrower than the output
    GS_WHY_CHANNELS,    // a channel count no instantiation takes
    GS_WHY_ALIGN,       // a base, a leading dimension or a channel count that breaks the kernels' 16-B (8-B) accesses
    GS_WHY_RES,         // kd_conv3x3_small: the same for its residual
    GS_WHY_TOO_LARGE,   // kd_conv3x3_small: more workgroups than a 32-bit grid
};

// What the kernels' translation units are built for; they alias these or static_assert against them.
constexpr int GS_SL_MAXC = 72;                                  // channels on either side of small_linear / small_wgrad
constexpr int GS_SL_TEMPLATES[] = {8, 16, 24, 40, GS_SL_MAXC};  // small_linear_kernel<COP>: the first that holds Cout
constexpr int GS_SW_CH = 64;                                    // pixels small_wgrad_partial_kernel stages at a time
constexpr int GS_SW_PIX_PER_BLOCK = 4096, GS_SW_MAX_BLOCKS = 1024;   // small_wgrad: >= 64 chunks a block, at most 1024 blocks
constexpr int GS_SC_SEG = 256, GS_SC_ROWS = 16;                 // conv3x3_small: a workgroup's row segment and output rows
constexpr int GS_SC_RING = 4;                                   // ... and the input rows its LDS ring holds
constexpr int GS_SC_THREADS_64 = 512, GS_THREADS = 256;         // conv3x3_small_kernel<64> runs eight waves, everything else four
constexpr int GS_SC_LDS_LIMIT = 64 * 1024;                      // dynamic LDS a kernel gets without its attribute raised
constexpr int GS_GC_PIX = 4, GS_GC_PIX_WIDE = 2, GS_GC_WIDE_C = 32;  // gated_conv_kernel: pixels a thread (its PIX): 2 from C = 32 on
constexpr int GS_MFMA_PIX = 16, GS_MFMA_WAVES = 4;              // the matrix-core kernels: pixels a wave and trip, waves a block
constexpr int GS_CANNY_GRAD_BYTES = 4, GS_CANNY_MAG_BYTES = 4, GS_CANNY_STATE_BYTES = 1, GS_CANNY_SLACK = 256;   // workspace per pixel: short2, int, byte
// grid caps of the grid-stride kernels, each tuned (or left) per call: the matrix-core kernels at 32 workgroups per CU
constexpr int GS_CAP_GATED_MFMA = 256 * 32, GS_CAP_POINTWISE_SMALL = 256 * 32;
constexpr int GS_CAP_GATED = 65536, GS_CAP_EDGE_ATTENTION = 65536, GS_CAP_EDGE_ASPP = 65536, GS_CAP_CANNY = 65536;
constexpr int GS_CAP_SMALL_LINEAR = 1 << 16, GS_CAP_GATE_MIX_BWD = 1 << 16, GS_CAP_EDGE_ATTENTION_BWD = 1 << 16, GS_CAP_RANK1_ADD = 1 << 20;

struct GsSel {
    GsKernel kernel;
    GsWhy why;
    unsigned grid, grid2;       // the first and (kd_small_wgrad: the finish) the second launch; all grids are one-dimensional
    int threads;                // per workgroup
    int lds;                    // dynamic LDS bytes
    bool raise_lds;             // the instantiation needs its dynamic-LDS attribute raised to `lds` before its first launch
    int sw_blocks;              // small_wgrad: blocks of the partial pass (= grid, = partials in the workspace)
    long long sw_per_block;     // ... and pixels each walks
    int nsx, nsy;               // conv3x3_small: row segments per image row, row groups per image
    float sh, sw;               // edge_aspp: source coordinate = output coordinate * s (align_corners)
    long long total;            // canny: pixels of the batch
    size_t ws_off[3];           // canny: byte offsets of the gradients, the magnitudes and the state in the workspace
};

// ---- predicates -----------------------------------------------------------------------------------------------------------------
static inline bool gs_dtype_ok(int d) { return d == KD_F32 || d == KD_BF16; }
static inline int gs_elem_size(int d) { return d == KD_BF16 ? 2 : 4; }
static inline bool gs_aligned(const void *p, unsigned bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }
// every pixel of the view starts 16-B aligned
static inline bool gs_rows16(const void *p, int ld, int es) { return gs_aligned(p, 16) && ((long long)ld * es) % 16 == 0; }
// a * b, or the largest value where that does not fit (every use is capped or compared right after)
static inline long long gs_mul(long long a, long long b)
{
    long long r;
    return __builtin_mul_overflow(a, b, &r) ? INT64_MAX : r;
}

// ---- grids ----------------------------------------------------------------------------------------------------------------------
// one thread per item, 256 a workgroup, at most `cap` workgroups (the kernels stride over the rest)
static inline unsigned gs_blocks(long long b, int cap) { return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b)); }
static inline unsigned gs_grid(long long total, int cap) { return gs_blocks(total / GS_THREADS + (total % GS_THREADS > 0), cap); }
static inline GsSel gs_flat(int kernel, unsigned blocks)
{
    GsSel c{};
    c.kernel = (GsKernel)kernel;
    c.grid = c.grid2 = blocks;
    c.threads = GS_THREADS;
    return c;
}
static inline GsSel gs_refuse(GsWhy why)
{
    GsSel c{};
    c.kernel = GS_REFUSED;
    c.why = why;
    return c;
}
// a 16-pixel group per wave and trip, four waves a workgroup
static inline unsigned gs_mfma_grid(long long npix, int cap)
{
    const long long waves = npix / GS_MFMA_PIX + (npix % GS_MFMA_PIX > 0);
    return gs_blocks((waves + GS_MFMA_WAVES - 1) / GS_MFMA_WAVES, cap);
}

// ---- gscnn_ops.hip --------------------------------------------------------------------------------------------------------------
static inline int gs_gated_pix(int C) { return C >= GS_GC_WIDE_C ? GS_GC_PIX_WIDE : GS_GC_PIX; }
// mfma: the process's KDCC_GATED_MFMA switch (on unless set to 0).  bf16 goes to the matrix cores whenever it is on -- the
// alignment they need is the alignment every call needs -- so the bf16 VALU instantiations are its other side only.
static inline GsSel gs_gated_conv(int dtype, const void *feat, int ldf, const void *out, int ldo, long long npix, int C, bool mfma)
{
    if (npix <= 0) return gs_refuse(GS_WHY_SHAPE);
    if (!gs_dtype_ok(dtype)) return gs_refuse(GS_WHY_DTYPE);
    if (C != 8 && C != 16 && C != 32) return gs_refuse(GS_WHY_CHANNELS);
    const int es = gs_elem_size(dtype), ci = C == 8 ? 0 : (C == 16 ? 1 : 2);
    if (!gs_rows16(feat, ldf, es) || !gs_rows16(out, ldo, es)) return gs_refuse(GS_WHY_ALIGN);
    if (mfma && dtype == KD_BF16) return gs_flat(GS_GATED_MFMA_8 + ci, gs_mfma_grid(npix, GS_CAP_GATED_MFMA));
    const int pix = gs_gated_pix(C);
    return gs_flat(GS_GATED_F32_8 + 3 * (dtype == KD_BF16) + ci, gs_grid(npix / pix + (npix % pix > 0), GS_CAP_GATED));
}
static inline GsSel gs_edge_attention(int dtype, const void *cs, int ldc, long long npix)
{
    if (npix <= 0) return gs_refuse(GS_WHY_SHAPE);
    if (!gs_dtype_ok(dtype)) return gs_refuse(GS_WHY_DTYPE);
    if (!gs_rows16(cs, ldc, gs_elem_size(dtype))) return gs_refuse(GS_WHY_ALIGN);
    return gs_flat(GS_EDGE_ATTENTION_F32 + (dtype == KD_BF16), gs_grid(npix, GS_CAP_EDGE_ATTENTION));
}
// a thread per output pixel and channel octet
static inline GsSel gs_edge_aspp(int dtype, const void *w, const void *scale, const void *shift, const void *y, int ldy, int N, int H, int W, int Ho,
                                 int Wo, int C)
{
    if (N <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || C <= 0) return gs_refuse(GS_WHY_SHAPE);
    if (!gs_dtype_ok(dtype)) return gs_refuse(GS_WHY_DTYPE);
    if (C % 8 != 0 || !gs_rows16(y, ldy, gs_elem_size(dtype)) || !gs_aligned(w, 16) || !gs_aligned(scale, 16) || !gs_aligned(shift, 16))
        return gs_refuse(GS_WHY_ALIGN);
    GsSel c = gs_flat(GS_EDGE_ASPP_F32 + (dtype == KD_BF16), gs_grid(gs_mul(gs_mul(gs_mul(N, Ho), Wo), C / 8), GS_CAP_EDGE_ASPP));
    const ResampleGeom g = resample_geom(H, W, Ho, Wo, 1);
    c.sh = g.sh; c.sw = g.sw;
    return c;
}
// workspace: short2 gradients | int magnitudes | byte states, N * H * W each, and 256 bytes of slack
static inline size_t gs_canny_workspace(int N, int H, int W)
{
    const size_t n = (size_t)N * H * W;
    return n * (GS_CANNY_GRAD_BYTES + GS_CANNY_MAG_BYTES + GS_CANNY_STATE_BYTES) + GS_CANNY_SLACK;
}
static inline GsSel gs_canny_plan(GsKernel kernel, int N, int H, int W)
{
    const long long n = gs_mul(gs_mul(N, H), W);
    GsSel c = gs_flat(kernel, gs_grid(n, GS_CAP_CANNY));
    c.total = n;
    c.ws_off[0] = 0;
    c.ws_off[1] = (size_t)n * GS_CANNY_GRAD_BYTES;
    c.ws_off[2] = c.ws_off[1] + (size_t)n * GS_CANNY_MAG_BYTES;
    return c;
}
static inline GsSel gs_canny(int N, int H, int W, int sweeps)
{
    return N > 0 && H > 0 && W > 0 && sweeps >= 0 ? gs_canny_plan(GS_CANNY, N, H, W) : gs_refuse(GS_WHY_SHAPE);
}
static inline GsSel gs_canny_continue(int N, int H, int W, int sweeps)
{
    return N > 0 && H > 0 && W > 0 && sweeps > 0 ? gs_canny_plan(GS_CANNY_CONTINUE, N, H, W) : gs_refuse(GS_WHY_SHAPE);
}
// grid: a workgroup per (image, group of GS_SC_ROWS rows, GS_SC_SEG-pixel row segment); lds: the ring of input rows, a halo pixel
// each side, C = 64 pixels padded by 16 B
static inline GsSel gs_conv3x3_small(const void *x, int ldx, const void *w, const void *res, int ldres, const void *y, int ldy, int N, int H, int W,
                                     int C)
{
    if (N <= 0 || H <= 0 || W <= 0) return gs_refuse(GS_WHY_SHAPE);
    if (C != 16 && C != 32 && C != 64) return gs_refuse(GS_WHY_CHANNELS);
    if (ldx < C || ldy < C || ldx % 8 != 0 || ldy % 8 != 0 || !gs_aligned(x, 16) || !gs_aligned(w, 16) || !gs_aligned(y, 16)) return gs_refuse(GS_WHY_ALIGN);
    if (res && (ldres < C || ldres % 8 != 0 || !gs_aligned(res, 16))) return gs_refuse(GS_WHY_RES);
    const int nsx = W / GS_SC_SEG + (W % GS_SC_SEG > 0), nsy = H / GS_SC_ROWS + (H % GS_SC_ROWS > 0);
    const long long blocks = gs_mul(gs_mul(N, nsx), nsy);
    if (blocks > 0x7fffffffLL) return gs_refuse(GS_WHY_TOO_LARGE);
    GsSel c = gs_flat(C == 64 ? GS_CONV3X3_64 : (C == 32 ? GS_CONV3X3_32 : GS_CONV3X3_16), (unsigned)blocks);
    c.threads = C == 64 ? GS_SC_THREADS_64 : GS_THREADS;
    c.lds = GS_SC_RING * (GS_SC_SEG + 2) * (C == 64 ? C * 2 + 16 : C * 2);
    c.raise_lds = c.lds > GS_SC_LDS_LIMIT;
    c.nsx = nsx;
    c.nsy = nsy;
    return c;
}
// x: 16-B aligned pixels; y: 8-B aligned channel quads
static inline GsSel gs_pointwise_small(const void *x, int ldx, const void *y, int ldy, long long npix, int Cin, int Cout)
{
    if (npix <= 0) return gs_refuse(GS_WHY_SHAPE);
    const int pair = Cin == 64 && Cout == 32 ? 0 : (Cin == 32 && Cout == 16 ? 1 : (Cin == 16 && Cout == 8 ? 2 : -1));
    if (pair < 0) return gs_refuse(GS_WHY_CHANNELS);
    if (ldx < Cin || ldy < Cout || ldx % 8 != 0 || ldy % 4 != 0 || !gs_aligned(x, 16) || !gs_aligned(y, 8)) return gs_refuse(GS_WHY_ALIGN);
    return gs_flat(GS_POINTWISE_64_32 + pair, gs_mfma_grid(npix, GS_CAP_POINTWISE_SMALL));
}

// ---- gscnn_bwd.hip --------------------------------------------------------------------------------------------------------------
static inline bool gs_small_channels_ok(int ld_in, int C_in, int ld_out, int C_out)
{
    return C_in >= 1 && C_in <= GS_SL_MAXC && C_out >= 1 && C_out <= GS_SL_MAXC && ld_in >= C_in && ld_out >= C_out;
}
static inline GsSel gs_small_linear(int x_dtype, int ldx, int Cin, int y_dtype, int ldy, int Cout, long long npix, const void *mask, int ldm)
{
    if (npix <= 0) return gs_refuse(GS_WHY_SHAPE);
    if (!gs_dtype_ok(x_dtype) || !gs_dtype_ok(y_dtype)) return gs_refuse(GS_WHY_DTYPE);
    if (mask && ldm < Cout) return gs_refuse(GS_WHY_MASK);
    if (!gs_small_channels_ok(ldx, Cin, ldy, Cout)) return gs_refuse(GS_WHY_CHANNELS);
    int t = 0;
    while (Cout > GS_SL_TEMPLATES[t]) ++t;      // ends: Cout <= GS_SL_MAXC, the last template
    return gs_flat(GS_SMALL_LINEAR_8 + t, gs_grid(npix, GS_CAP_SMALL_LINEAR));
}
// >= 64 chunks of 64 pixels per block, at most 1024 blocks; a block's pixels are whole chunks, which may leave fewer blocks
static inline int gs_small_wgrad_blocks(long long npix, long long *per_block)
{
    long long nb = npix / GS_SW_PIX_PER_BLOCK + (npix % GS_SW_PIX_PER_BLOCK > 0);
    if (nb > GS_SW_MAX_BLOCKS) nb = GS_SW_MAX_BLOCKS;
    if (nb < 1) nb = 1;
    long long pb = npix / nb + (npix % nb > 0);
    pb = (pb / GS_SW_CH + (pb % GS_SW_CH > 0)) * GS_SW_CH;
    *per_block = pb;
    return (int)(npix / pb + (npix % pb > 0));
}
// one (Cb * Ca + Cb) fp32 partial per block
static inline size_t gs_small_wgrad_workspace(int Ca, int Cb, long long npix)
{
    if (Ca < 1 || Cb < 1 || npix < 1) return 0;
    long long pb;
    return (size_t)gs_small_wgrad_blocks(npix, &pb) * ((size_t)Ca * Cb + Cb) * sizeof(float);
}
// grid: the partial pass; grid2: the fixed-order finish, a thread per weight and bias element
static inline GsSel gs_small_wgrad(int a_dtype, int lda, int Ca, int b_dtype, int ldb, int Cb, long long npix)
{
    if (npix <= 0) return gs_refuse(GS_WHY_SHAPE);
    if (!gs_dtype_ok(a_dtype) || !gs_dtype_ok(b_dtype)) return gs_refuse(GS_WHY_DTYPE);
    if (!gs_small_channels_ok(lda, Ca, ldb, Cb)) return gs_refuse(GS_WHY_CHANNELS);
    GsSel c = gs_flat(GS_SMALL_WGRAD, 1);
    c.sw_blocks = gs_small_wgrad_blocks(npix, &c.sw_per_block);
    c.grid = (unsigned)c.sw_blocks;
    c.grid2 = (unsigned)((Ca * Cb + Cb + GS_THREADS - 1) / GS_THREADS);
    return c;
}
static inline GsSel gs_gate_mix_bwd(int feat_dtype, int C, long long npix)
{
    if (npix <= 0 || C < 1) return gs_refuse(GS_WHY_SHAPE);
    if (!gs_dtype_ok(feat_dtype)) return gs_refuse(GS_WHY_DTYPE);
    return gs_flat(GS_GATE_MIX_BWD, gs_grid(npix, GS_CAP_GATE_MIX_BWD));
}
static inline GsSel gs_edge_attention_bwd(int dtype, int ldc, long long npix)
{
    if (npix <= 0) return gs_refuse(GS_WHY_SHAPE);
    if (!gs_dtype_ok(dtype) || ldc < 8) return gs_refuse(GS_WHY_DTYPE);
    return gs_flat(GS_EDGE_ATTENTION_BWD, gs_grid(npix, GS_CAP_EDGE_ATTENTION_BWD));
}
// a thread per pixel and channel octet
static inline GsSel gs_rank1_add(int dtype, const void *y, int ldy, const void *w, int C, long long npix)
{
    if (npix <= 0 || C <= 0) return gs_refuse(GS_WHY_SHAPE);
    if (!gs_dtype_ok(dtype)) return gs_refuse(GS_WHY_DTYPE);
    if (C % 8 != 0 || !gs_rows16(y, ldy, gs_elem_size(dtype)) || !gs_aligned(w, 16)) return gs_refuse(GS_WHY_ALIGN);
    return gs_flat(GS_RANK1_ADD_F32 + (dtype == KD_BF16), gs_grid(gs_mul(npix, C / 8), GS_CAP_RANK1_ADD));
}
