// Dropout on an (M, C) NHWC view: y = keep ? x * scale : 0, the keep decision the counter-based rule of dropout_rng.h -- a pure
// function of (seed, offset, m * C + c) -- so the same entry point with the same pair is the backward (dx = dropout(gy)) and nothing
// is stored between the two.  One elementwise pass, HBM-bound at the sizes it is meant for; no workspace, no atomics, no LDS.
//
// dropout_vec_kernel<T, V>: a lane owns V = 16 B / sizeof(T) consecutive channels of one pixel: one 16-B load, one 16-B store.  With
// C % V == 0 the group's first index (m * (C / V) + g) * V is the item number times V, a multiple of 4: the lane's channels are
// exactly 1 (fp32) or 2 (bf16) Philox blocks, no word is generated twice or thrown away.
// dropout_block_kernel<T>: a lane owns one Philox block, the 4 consecutive indices 4q .. 4q + 3, which may run over the end of a
// pixel into the next one (and stop at M * C): scalar loads and stores, any C, any stride, any element-aligned base.
// Both stride over their items on a capped grid.  A lane loads its elements before it stores them and touches no others, so x == y
// is allowed, and channels [C, ld) of a padded view are neither read nor written.  Which one runs is dropout_select.h's decision.
#include "dropout_rng.h"
#include "dropout_select.h"
#include "kd_common.h"

namespace {

constexpr int TPB = DROPOUT_TPB;
static_assert(TPB % 64 == 0 && DROPOUT_BLOCK == DROPOUT_WORDS, "a scalar lane owns one Philox block");

// item -> (pixel, group within the pixel); a 32-bit division while the item number fits one
__device__ __forceinline__ void split(long long i, int G, long long &m, int &g)
{
    if ((i >> 32) == 0) {
        const uint32_t q = (uint32_t)i / (uint32_t)G;
        m = q;
        g = (int)((uint32_t)i - q * (uint32_t)G);
    } else {
        m = i / G;
        g = (int)(i - m * G);
    }
}

template <typename T, int V>
__global__ __launch_bounds__(TPB) void dropout_vec_kernel(const T *x, int ldx, T *y, int ldy, long long items, int C, uint32_t threshold, float scale,
                                                          uint64_t seed, uint64_t offset)
{
    static_assert(V * sizeof(T) == DROPOUT_VEC_BYTES && V % DROPOUT_WORDS == 0, "a lane owns 16 B: whole Philox blocks");
    const int G = C / V;
    const long long step = (long long)gridDim.x * TPB;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < items; i += step) {
        long long m;
        int g;
        split(i, G, m, g);
        const int c = g * V;
        float v[V];
        if constexpr (V == 4) {
            const float4 a = *(const float4 *)(x + m * ldx + c);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        } else {
            ld8(x + m * ldx + c, v);
        }
#pragma unroll
        for (int b = 0; b < V / DROPOUT_WORDS; ++b) {
            const PhiloxBlock r = dropout_block(seed, offset, i * (V / DROPOUT_WORDS) + b);      // (m * C + c) >> 2, + b
#pragma unroll
            for (int j = 0; j < DROPOUT_WORDS; ++j)
                v[b * DROPOUT_WORDS + j] = dropout_apply(v[b * DROPOUT_WORDS + j], dropout_keep_word(r.w[j], threshold), scale);
        }
        if constexpr (V == 4) *(float4 *)(y + m * ldy + c) = make_float4(v[0], v[1], v[2], v[3]);
        else st8(y + m * ldy + c, v);
    }
}

template <typename T>
__global__ __launch_bounds__(TPB) void dropout_block_kernel(const T *x, int ldx, T *y, int ldy, long long items, long long total, int C,
                                                            uint32_t threshold, float scale, uint64_t seed, uint64_t offset)
{
    const long long step = (long long)gridDim.x * TPB;
    for (long long q = (long long)blockIdx.x * TPB + threadIdx.x; q < items; q += step) {
        const long long idx0 = q * DROPOUT_WORDS;
        long long m;
        int c;
        split(idx0, C, m, c);
        const PhiloxBlock r = dropout_block(seed, offset, q);
        float v[DROPOUT_WORDS];
        long long mj = m;
        int cj = c;
#pragma unroll
        for (int j = 0; j < DROPOUT_WORDS; ++j) {          // every load of the lane before its first store
            v[j] = idx0 + j < total ? Elem<T>::ld(x + mj * ldx + cj) : 0.f;
            if (++cj == C) { cj = 0; ++mj; }
        }
        mj = m; cj = c;
#pragma unroll
        for (int j = 0; j < DROPOUT_WORDS; ++j) {
            if (idx0 + j < total) Elem<T>::st(y + mj * ldy + cj, dropout_apply(v[j], dropout_keep_word(r.w[j], threshold), scale));
            if (++cj == C) { cj = 0; ++mj; }
        }
    }
}

}  // namespace

extern "C" int kd_dropout_nhwc(const void *x, int32_t ldx, void *y, int32_t ldy, int32_t dtype, int64_t M, int32_t C, uint32_t threshold,
                               float scale, uint64_t seed, uint64_t offset, kd_stream_t stream)
{
    KD_REQUIRE(dropout_args_ok(x, ldx, y, ldy, dtype, M, C), KD_ERR_INVALID,
               "kd_dropout_nhwc: dtype %d, M = %lld, C = %d, pixel strides %d / %d, or a null or misaligned operand", (int)dtype, (long long)M,
               (int)C, (int)ldx, (int)ldy);
    const DropoutSel sel = dropout_select(dtype, M, C, x, ldx, y, ldy);
    KD_NOTE_PLUMBING(dropout_kernel_name(sel.kernel));
    const dim3 grid(sel.grid), block(TPB);
    hipStream_t s = (hipStream_t)stream;
    const long long total = (long long)M * C;
    switch (sel.kernel) {
    case DK_F32_V:
        hipLaunchKernelGGL((dropout_vec_kernel<float, 4>), grid, block, 0, s, (const float *)x, ldx, (float *)y, ldy, sel.items, C, threshold, scale,
                           seed, offset);
        break;
    case DK_BF16_V:
        hipLaunchKernelGGL((dropout_vec_kernel<bf16_t, 8>), grid, block, 0, s, (const bf16_t *)x, ldx, (bf16_t *)y, ldy, sel.items, C, threshold,
                           scale, seed, offset);
        break;
    case DK_F32_1:
        hipLaunchKernelGGL((dropout_block_kernel<float>), grid, block, 0, s, (const float *)x, ldx, (float *)y, ldy, sel.items, total, C, threshold,
                           scale, seed, offset);
        break;
    default:
        hipLaunchKernelGGL((dropout_block_kernel<bf16_t>), grid, block, 0, s, (const bf16_t *)x, ldx, (bf16_t *)y, ldy, sel.items, total, C,
                           threshold, scale, seed, offset);
        break;
    }
    KD_CHECK_LAUNCH("kd_dropout_nhwc");
    return KD_OK;
}
