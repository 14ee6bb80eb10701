// HRNetV2-W48 + OCR pieces that no other kernel of the library covers (models/hrnet_ocr/seg_hrnet_ocr.py of the reference):
//   * the multi-resolution fuse sum of HighResolutionModule.forward (:399-414): y = relu(sum_s resample(src_s)), one pass that
//     writes y once, and its backward (ReLU mask, identity for a same-resolution source, the bilinear adjoint in gather form
//     for a coarser one);
//   * SpatialGather_Module (:65-73): ctx = softmax_HW(logits)^T . feats over K <= 32 classes;
//   * the core of _ObjectAttentionBlock.forward (:138-143): ctx = softmax_K(scale * q . key^T) . value.
// All fp32 NHWC, wave64, 16-byte accesses along the channel axis (C % 4 == 0), no float atomics: every reduction over pixels
// goes through per-chunk partial sums in a workspace that a second kernel adds in chunk order, so results are bit-reproducible.
#include "kd_common.h"
#include "resample.h"

#include <math.h>

namespace {

constexpr int HR_MAX_SRC = 4;
constexpr int OCR_MAX_K = 32;
constexpr int OCR_TILE = 64;            // pixels whose K weights one block stages in LDS at a time
constexpr size_t OCR_LDS_LIMIT = 64 * 1024;

__device__ __forceinline__ float4 f4_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 f4_fma(float a, float4 b, float4 c)
{
    return make_float4(fmaf(a, b.x, c.x), fmaf(a, b.y, c.y), fmaf(a, b.z, c.z), fmaf(a, b.w, c.w));
}
__device__ __forceinline__ float4 f4_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float f4_dot(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float4 resample_lerp(float f, float4 a, float4 b)
{
    return make_float4(::resample_lerp(f, a.x, b.x), ::resample_lerp(f, a.y, b.y), ::resample_lerp(f, a.z, b.z), ::resample_lerp(f, a.w, b.w));
}

// ---------------------------------------------------------------------------------------------------------------- fuse sum
struct HrSrc {
    float *x;          // source (forward) / source gradient (backward)
    int H, W, ld;
    float sh, sw;      // align_corners=True scales (resample_geom)
    long long first;   // backward: index of this source's first work item
};
struct HrArgs {
    HrSrc s[HR_MAX_SRC];
    int n;
};

// one thread per (n, ho, wo, 4 channels)
__global__ __launch_bounds__(256) void hr_fuse_fwd_kernel(HrArgs a, float *__restrict__ y, int ldy, int N, int Ho, int Wo, int C4)
{
    const long long total = (long long)N * Ho * Wo * C4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C4) * 4;
    long long r = i / C4;
    const int wo = (int)(r % Wo); r /= Wo;
    const int ho = (int)(r % Ho);
    const int n = (int)(r / Ho);
    float4 acc = f4_zero();
#pragma unroll
    for (int s = 0; s < HR_MAX_SRC; ++s) {
        if (s >= a.n) break;
        const HrSrc &S = a.s[s];
        const float *b = S.x + (size_t)n * S.H * S.W * S.ld + c;
        float4 v;
        if (S.H == Ho && S.W == Wo) {
            v = *(const float4 *)(b + ((size_t)ho * Wo + wo) * S.ld);
        } else {
            int h0, h1, w0, w1; float ah, aw;
            resample_src(ho, S.sh, S.H, h0, h1, ah);
            resample_src(wo, S.sw, S.W, w0, w1, aw);
            const float4 t = resample_lerp(aw, *(const float4 *)(b + ((size_t)h0 * S.W + w0) * S.ld), *(const float4 *)(b + ((size_t)h0 * S.W + w1) * S.ld));
            const float4 u = resample_lerp(aw, *(const float4 *)(b + ((size_t)h1 * S.W + w0) * S.ld), *(const float4 *)(b + ((size_t)h1 * S.W + w1) * S.ld));
            v = resample_lerp(ah, t, u);
        }
        acc = s == 0 ? v : f4_add(acc, v);
    }
    acc.x = fmaxf(acc.x, 0.f); acc.y = fmaxf(acc.y, 0.f); acc.z = fmaxf(acc.z, 0.f); acc.w = fmaxf(acc.w, 0.f);
    *(float4 *)(y + (((size_t)n * Ho + ho) * Wo + wo) * ldy + c) = acc;
}

__device__ __forceinline__ float4 hr_masked(const float *gy, const float *y, size_t og, size_t oy)
{
    const float4 g = *(const float4 *)(gy + og), v = *(const float4 *)(y + oy);
    return make_float4(v.x > 0.f ? g.x : 0.f, v.y > 0.f ? g.y : 0.f, v.z > 0.f ? g.z : 0.f, v.w > 0.f ? g.w : 0.f);
}

// one thread per (source, n, h, w, 4 channels) of the sources whose gradient is wanted; a.s[].x are the gradient buffers
__global__ __launch_bounds__(256) void hr_fuse_bwd_kernel(HrArgs a, long long total, const float *__restrict__ gy, int ldgy,
                                                          const float *__restrict__ y, int ldy, int N, int Ho, int Wo, int C4)
{
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int s = 0;
#pragma unroll
    for (int q = 1; q < HR_MAX_SRC; ++q)
        if (q < a.n && i >= a.s[q].first) s = q;
    const HrSrc S = a.s[s];
    i -= S.first;
    const int c = (int)(i % C4) * 4;
    long long r = i / C4;
    const int w = (int)(r % S.W); r /= S.W;
    const int h = (int)(r % S.H);
    const int n = (int)(r / S.H);
    float4 acc;
    if (S.H == Ho && S.W == Wo) {
        const size_t p = ((size_t)n * Ho + h) * Wo + w;
        acc = hr_masked(gy, y, p * ldgy + c, p * ldy + c);
    } else {
        acc = f4_zero();
        int hlo, hhi, wlo, whi;
        resample_adjoint_range(h, S.sh, 0.f, Ho, hlo, hhi);
        resample_adjoint_range(w, S.sw, 0.f, Wo, wlo, whi);
        for (int ho = hlo; ho <= hhi; ++ho) {
            const float wh = resample_adjoint_weight(ho, h, S.sh, S.H);
            if (wh == 0.f) continue;
            for (int wo = wlo; wo <= whi; ++wo) {
                const float ww = resample_adjoint_weight(wo, w, S.sw, S.W);
                if (ww == 0.f) continue;
                const size_t p = ((size_t)n * Ho + ho) * Wo + wo;
                acc = f4_fma(wh * ww, hr_masked(gy, y, p * ldgy + c, p * ldy + c), acc);
            }
        }
    }
    *(float4 *)(S.x + (((size_t)n * S.H + h) * S.W + w) * S.ld + c) = acc;
}

// ---------------------------------------------------------------------------------------------------------------- OCR
// Pixel chunks of the two-stage reductions over HW: at most 32 chunks of a multiple of OCR_TILE pixels.
struct Chunks {
    int count, per;
};
inline Chunks ocr_chunks(long long HW)
{
    long long pc = (HW + OCR_TILE - 1) / OCR_TILE;
    if (pc > 32) pc = 32;
    long long per = ((HW + pc - 1) / pc + OCR_TILE - 1) / OCR_TILE * OCR_TILE;
    Chunks c;
    c.per = (int)per;
    c.count = (int)((HW + per - 1) / per);
    return c;
}

// combine two (max, sum of exp(v - max)) pairs; an empty side is (-inf, 0)
__device__ __forceinline__ void lse_merge(float &m, float &s, float m2, float s2)
{
    const float M = fmaxf(m, m2);
    if (M == -INFINITY) { s = 0.f; return; }
    s = s * expf(m - M) + s2 * expf(m2 - M);
    m = M;
}

// stage 1 of the softmax statistics over HW: grid (chunks, N); stat[(n * chunks + chunk) * K + k] = (max, sum)
__global__ __launch_bounds__(256) void ocr_stats_kernel(const float *__restrict__ logits, int ldl, float2 *__restrict__ stat, int HW, int K, int per)
{
    __shared__ float2 sh[4][OCR_MAX_K];
    const int chunk = blockIdx.x, n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p0 = chunk * per, p1 = min(HW, p0 + per);
    float m[OCR_MAX_K], s[OCR_MAX_K];
#pragma unroll
    for (int k = 0; k < OCR_MAX_K; ++k) { m[k] = -INFINITY; s[k] = 0.f; }
    for (int p = p0 + (int)threadIdx.x; p < p1; p += 256) {
        const float *row = logits + ((size_t)n * HW + p) * ldl;
#pragma unroll
        for (int k = 0; k < OCR_MAX_K; ++k)
            if (k < K) lse_merge(m[k], s[k], row[k], 1.f);
    }
#pragma unroll
    for (int k = 0; k < OCR_MAX_K; ++k) {
        if (k < K) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float m2 = __shfl_xor(m[k], o, 64), s2 = __shfl_xor(s[k], o, 64);
                lse_merge(m[k], s[k], m2, s2);
            }
            if (lane == 0) sh[wave][k] = make_float2(m[k], s[k]);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {
        float2 a = sh[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) lse_merge(a.x, a.y, sh[w][threadIdx.x].x, sh[w][threadIdx.x].y);
        stat[((size_t)n * gridDim.x + chunk) * K + threadIdx.x] = a;
    }
}

// stage 2: grid N, 64 threads; mx[n][k], lse[n][k] = max + log(sum), chunks merged in order
__global__ __launch_bounds__(64) void ocr_stats_finish_kernel(const float2 *__restrict__ stat, float *__restrict__ mx, float *__restrict__ lse, int K, int chunks)
{
    const int n = blockIdx.x, k = threadIdx.x;
    if (k >= K) return;
    float2 a = stat[((size_t)n * chunks) * K + k];
    for (int c = 1; c < chunks; ++c) {
        const float2 b = stat[((size_t)n * chunks + c) * K + k];
        lse_merge(a.x, a.y, b.x, b.y);
    }
    mx[(size_t)n * K + k] = a.x;
    lse[(size_t)n * K + k] = a.x + logf(a.y);
}

// part[((n * chunks + chunk) * K + k) * C + c] = sum over the chunk's pixels p of wgt(p, k) * f[p][c];
// SOFTMAX: wgt = exp(w[p][k] - lse[n][k]) (the probability, recomputed), else wgt = w[p][k].
// grid (chunks, ceil(C / 256), N); a lane owns 4 channels, the 4 waves of a block take every fourth pixel of a 64-pixel tile
// whose K weights are staged in LDS once, and are added in wave order at the end.
template <bool SOFTMAX>
__global__ __launch_bounds__(256) void ocr_contract_kernel(const float *__restrict__ w, int ldw, const float *__restrict__ lse,
                                                           const float *__restrict__ f, int ldf, float *__restrict__ part, int HW, int K,
                                                           int C, int per)
{
    __shared__ float pr[OCR_TILE][OCR_MAX_K];
    __shared__ float4 red[3][64];
    const int chunk = blockIdx.x, n = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = (blockIdx.y * 64 + lane) * 4;
    const bool cvalid = c < C;
    const int p0 = chunk * per, p1 = min(HW, p0 + per);
    float4 acc[OCR_MAX_K];
#pragma unroll
    for (int k = 0; k < OCR_MAX_K; ++k) acc[k] = f4_zero();
    for (int t0 = p0; t0 < p1; t0 += OCR_TILE) {
        __syncthreads();
        for (int i = threadIdx.x; i < OCR_TILE * K; i += 256) {
            const int pp = i / K, k = i - pp * K, p = t0 + pp;
            float v = 0.f;
            if (p < p1) {
                v = w[((size_t)n * HW + p) * ldw + k];
                if (SOFTMAX) v = expf(v - lse[(size_t)n * K + k]);
            }
            pr[pp][k] = v;
        }
        __syncthreads();
        const int cnt = min(OCR_TILE, p1 - t0);
        for (int j = wave; j < cnt; j += 4) {
            const float4 v = cvalid ? *(const float4 *)(f + ((size_t)n * HW + t0 + j) * ldf + c) : f4_zero();
#pragma unroll
            for (int k = 0; k < OCR_MAX_K; ++k)
                if (k < K) acc[k] = f4_fma(pr[j][k], v, acc[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < OCR_MAX_K; ++k) {
        if (k < K) {                         // (K is block-uniform: every thread reaches the barriers)
            __syncthreads();
            if (wave > 0) red[wave - 1][lane] = acc[k];
            __syncthreads();
            if (wave == 0 && cvalid) {
                const float4 r = f4_add(f4_add(f4_add(acc[k], red[0][lane]), red[1][lane]), red[2][lane]);
                *(float4 *)(part + (((size_t)n * gridDim.x + chunk) * K + k) * C + c) = r;
            }
        }
    }
}

// out[n][k][c] = sum_chunk part[n][chunk][k][c], chunks in order; one thread per 4 channels
__global__ __launch_bounds__(256) void ocr_contract_finish_kernel(const float *__restrict__ part, float *__restrict__ out, int N, int K, int C, int chunks)
{
    const int C4 = C / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)N * K * C4) return;
    const int c = (int)(i % C4) * 4;
    const long long nk = i / C4;
    const int k = (int)(nk % K), n = (int)(nk / K);
    float4 a = f4_zero();
    for (int q = 0; q < chunks; ++q) a = f4_add(a, *(const float4 *)(part + (((size_t)n * chunks + q) * K + k) * C + c));
    *(float4 *)(out + ((size_t)n * K + k) * C + c) = a;
}

// dk[n][k] = sum_c a[n][k][c] * b[n][k][c]; grid N * K, one wave
__global__ __launch_bounds__(64) void ocr_rowdot_kernel(const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ dk, int C)
{
    const size_t row = (size_t)blockIdx.x * C;
    float s = 0.f;
    for (int c = threadIdx.x * 4; c < C; c += 256) s += f4_dot(*(const float4 *)(a + row + c), *(const float4 *)(b + row + c));
    s = wave_sum(s);
    if (threadIdx.x == 0) dk[blockIdx.x] = s;
}

__device__ __forceinline__ void lds_fill(float *dst, const float *src, int count4)
{
    for (int i = threadIdx.x; i < count4; i += 256) ((float4 *)dst)[i] = ((const float4 *)src)[i];
}

// Backward of the spatial gather.  p[pix][k] = exp(l - lse[k]);  d_feats[pix] = sum_k p[k] gctx[k];
// d_logits[pix][k] = p[k] * (<gctx[k], f[pix]> - dk[k]) with dk[k] = <gctx[k], ctx[k]> (the softmax-over-HW Jacobian).
// grid (blocks of `per` pixels, N); gctx[n] (K x C) sits in LDS; a wave takes two pixels at a time, lanes own 4 channels.
__global__ __launch_bounds__(256) void ocr_gather_bwd_kernel(const float *__restrict__ gctx, const float *__restrict__ dk,
                                                             const float *__restrict__ logits, int ldl, const float *__restrict__ feats, int ldf,
                                                             const float *__restrict__ lse, float *__restrict__ dfeats, int lddf,
                                                             float *__restrict__ dlogits, int lddl, int HW, int K, int C, int per)
{
    extern __shared__ __attribute__((aligned(16))) float panel[];
    const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    lds_fill(panel, gctx + (size_t)n * K * C, K * C / 4);
    __syncthreads();
    const int p0 = blockIdx.x * per, p1 = min(HW, p0 + per);
    const float my_lse = lane < K ? lse[(size_t)n * K + lane] : 0.f, my_dk = lane < K ? dk[(size_t)n * K + lane] : 0.f;
    for (int pa = p0 + wave * 2; pa < p1; pa += 8) {
        const bool two = pa + 1 < p1;
        const int pb = two ? pa + 1 : pa;
        const size_t ra = (size_t)n * HW + pa, rb = (size_t)n * HW + pb;
        const float pra = lane < K ? expf(logits[ra * ldl + lane] - my_lse) : 0.f;
        const float prb = lane < K ? expf(logits[rb * ldl + lane] - my_lse) : 0.f;
        float pka[OCR_MAX_K], pkb[OCR_MAX_K], dpa[OCR_MAX_K], dpb[OCR_MAX_K];
#pragma unroll
        for (int k = 0; k < OCR_MAX_K; ++k) {
            pka[k] = __shfl(pra, k, 64); pkb[k] = __shfl(prb, k, 64);
            dpa[k] = 0.f; dpb[k] = 0.f;
        }
        for (int c = lane * 4; c < C; c += 256) {
            const float4 fa = *(const float4 *)(feats + ra * ldf + c), fb = *(const float4 *)(feats + rb * ldf + c);
            float4 da = f4_zero(), db = f4_zero();
#pragma unroll
            for (int k = 0; k < OCR_MAX_K; ++k) {
                if (k < K) {
                    const float4 g = *(const float4 *)(panel + (size_t)k * C + c);
                    dpa[k] += f4_dot(fa, g); dpb[k] += f4_dot(fb, g);
                    da = f4_fma(pka[k], g, da); db = f4_fma(pkb[k], g, db);
                }
            }
            *(float4 *)(dfeats + ra * lddf + c) = da;
            if (two) *(float4 *)(dfeats + rb * lddf + c) = db;
        }
        float outa = 0.f, outb = 0.f;
#pragma unroll
        for (int k = 0; k < OCR_MAX_K; ++k) {
            if (k < K) {
                const float sa = wave_sum(dpa[k]), sb = wave_sum(dpb[k]);
                if (lane == k) { outa = sa; outb = sb; }
            }
        }
        if (lane < K) {
            dlogits[ra * lddl + lane] = pra * (outa - my_dk);
            if (two) dlogits[rb * lddl + lane] = prb * (outb - my_dk);
        }
    }
}

// Object attention.  grid (blocks of `per` pixels, N); key[n] and value[n] (K x Ck each) sit in LDS; a wave takes one pixel,
// lanes own 4 channels; the K scores of the pixel are wave sums every lane holds, so the softmax over K is register work.
// BWD: also reads g = d ctx, writes dq and, for the two reductions over HW that follow, p and ds = scale * p * (dp - <p, dp>).
template <bool BWD>
__global__ __launch_bounds__(256) void ocr_attend_kernel(const float *__restrict__ q, int ldq, const float *__restrict__ key,
                                                         const float *__restrict__ value, float *__restrict__ out, int ldo,
                                                         const float *__restrict__ g, int ldg, float *__restrict__ wp, float *__restrict__ wds,
                                                         int HW, int K, int Ck, float scale, int per)
{
    extern __shared__ __attribute__((aligned(16))) float panel[];
    float *kp = panel, *vp = panel + (size_t)K * Ck;
    const int n = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    lds_fill(kp, key + (size_t)n * K * Ck, K * Ck / 4);
    lds_fill(vp, value + (size_t)n * K * Ck, K * Ck / 4);
    __syncthreads();
    const int p0 = blockIdx.x * per, p1 = min(HW, p0 + per);
    for (int p = p0 + wave; p < p1; p += 4) {
        const size_t row = (size_t)n * HW + p;
        float s[OCR_MAX_K], dp[OCR_MAX_K];
#pragma unroll
        for (int k = 0; k < OCR_MAX_K; ++k) { s[k] = 0.f; dp[k] = 0.f; }
        for (int c = lane * 4; c < Ck; c += 256) {
            const float4 qv = *(const float4 *)(q + row * ldq + c);
            float4 gv = f4_zero();
            if (BWD) gv = *(const float4 *)(g + row * ldg + c);
#pragma unroll
            for (int k = 0; k < OCR_MAX_K; ++k) {
                if (k < K) {
                    s[k] += f4_dot(qv, *(const float4 *)(kp + (size_t)k * Ck + c));
                    if (BWD) dp[k] += f4_dot(gv, *(const float4 *)(vp + (size_t)k * Ck + c));
                }
            }
        }
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < OCR_MAX_K; ++k) {
            if (k < K) {
                s[k] = wave_sum(s[k]) * scale;
                if (BWD) dp[k] = wave_sum(dp[k]);
                m = fmaxf(m, s[k]);
            }
        }
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < OCR_MAX_K; ++k)
            if (k < K) { s[k] = expf(s[k] - m); sum += s[k]; }
        const float inv = 1.f / sum;
        float pd = 0.f;
#pragma unroll
        for (int k = 0; k < OCR_MAX_K; ++k)
            if (k < K) { s[k] *= inv; if (BWD) pd += s[k] * dp[k]; }
        if (BWD) {
            float myp = 0.f, myds = 0.f;
#pragma unroll
            for (int k = 0; k < OCR_MAX_K; ++k) {
                if (k < K) {
                    dp[k] = scale * s[k] * (dp[k] - pd);      // ds (with the score scale folded in)
                    if (lane == k) { myp = s[k]; myds = dp[k]; }
                }
            }
            if (lane < K) { wp[row * K + lane] = myp; wds[row * K + lane] = myds; }
        }
        for (int c = lane * 4; c < Ck; c += 256) {
            float4 o = f4_zero();
#pragma unroll
            for (int k = 0; k < OCR_MAX_K; ++k) {
                if (k < K) {
                    if (BWD) o = f4_fma(dp[k], *(const float4 *)(kp + (size_t)k * Ck + c), o);
                    else o = f4_fma(s[k], *(const float4 *)(vp + (size_t)k * Ck + c), o);
                }
            }
            *(float4 *)(out + row * ldo + c) = o;
        }
    }
}

inline size_t pad4(size_t n) { return (n + 3) & ~(size_t)3; }      // workspace sections start 16-byte aligned
inline bool ok4(const void *p, int ld) { return kd_aligned16(p) && ld % 4 == 0; }

// pixels per block of the per-pixel kernels: enough blocks to fill the chip, a multiple of 8 (4 waves x 2 pixels)
inline int ocr_pixels_per_block(long long HW)
{
    long long per = (HW + 127) / 128;
    per = (per + 7) / 8 * 8;
    return (int)per;
}

int fill_args(HrArgs &a, const kd_hr_view *v, int nsrc, int Ho, int Wo, int C, const char *who)
{
    a.n = 0;
    for (int s = 0; s < nsrc; ++s) {
        if (!v[s].ptr) continue;
        KD_REQUIRE(v[s].H > 0 && v[s].W > 0 && v[s].H <= Ho && v[s].W <= Wo && v[s].ld >= C && ok4(v[s].ptr, v[s].ld), KD_ERR_INVALID,
                   "%s: source %d must be no finer than the output, 16-byte aligned, ld %% 4 == 0 and ld >= C", who, s);
        HrSrc &S = a.s[a.n++];
        S.x = (float *)v[s].ptr; S.H = v[s].H; S.W = v[s].W; S.ld = v[s].ld;
        const ResampleGeom g = resample_geom(S.H, S.W, Ho, Wo, 1);
        S.sh = g.sh; S.sw = g.sw;
        S.first = 0;
    }
    return KD_OK;
}

}  // namespace

extern "C" int kd_hr_fuse_fwd(const kd_hr_view *src, int32_t nsrc, void *y, int32_t ldy, int32_t N, int32_t Ho, int32_t Wo, int32_t C,
                              kd_stream_t stream)
{
    KD_REQUIRE(src && y && nsrc >= 1 && nsrc <= HR_MAX_SRC && N > 0 && Ho > 0 && Wo > 0 && C > 0, KD_ERR_INVALID, "kd_hr_fuse_fwd: bad argument");
    KD_REQUIRE(C % 4 == 0 && ok4(y, ldy) && ldy >= C, KD_ERR_UNSUPPORTED, "kd_hr_fuse_fwd: C %% 4 == 0 and 16-byte aligned views required");
    for (int s = 0; s < nsrc; ++s) KD_REQUIRE(src[s].ptr, KD_ERR_INVALID, "kd_hr_fuse_fwd: null source");
    HrArgs a;
    const int rc = fill_args(a, src, nsrc, Ho, Wo, C, "kd_hr_fuse_fwd");
    if (rc != KD_OK) return rc;
    const long long total = (long long)N * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(hr_fuse_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, (float *)y, ldy, N, Ho, Wo, C / 4);
    KD_CHECK_LAUNCH("kd_hr_fuse_fwd");
    return KD_OK;
}

extern "C" int kd_hr_fuse_bwd(const void *gy, int32_t ldgy, const void *y, int32_t ldy, const kd_hr_view *gsrc, int32_t nsrc, int32_t N,
                              int32_t Ho, int32_t Wo, int32_t C, kd_stream_t stream)
{
    KD_REQUIRE(gy && y && gsrc && nsrc >= 1 && nsrc <= HR_MAX_SRC && N > 0 && Ho > 0 && Wo > 0 && C > 0, KD_ERR_INVALID, "kd_hr_fuse_bwd: bad argument");
    KD_REQUIRE(C % 4 == 0 && ok4(gy, ldgy) && ok4(y, ldy) && ldgy >= C && ldy >= C, KD_ERR_UNSUPPORTED,
               "kd_hr_fuse_bwd: C %% 4 == 0 and 16-byte aligned views required");
    HrArgs a;
    const int rc = fill_args(a, gsrc, nsrc, Ho, Wo, C, "kd_hr_fuse_bwd");
    if (rc != KD_OK) return rc;
    if (a.n == 0) return KD_OK;              // nobody needs a gradient
    long long total = 0;
    for (int s = 0; s < a.n; ++s) {
        a.s[s].first = total;
        total += (long long)N * a.s[s].H * a.s[s].W * (C / 4);
    }
    hipLaunchKernelGGL(hr_fuse_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, total, (const float *)gy, ldgy,
                       (const float *)y, ldy, N, Ho, Wo, C / 4);
    KD_CHECK_LAUNCH("kd_hr_fuse_bwd");
    return KD_OK;
}

extern "C" size_t kd_ocr_gather_workspace(int32_t N, int64_t HW, int32_t K, int32_t C)
{
    const Chunks ch = ocr_chunks(HW);
    // softmax statistics per chunk (float2) | context partial sums per chunk; the backward's N * K row dots fit in the first part
    return (pad4((size_t)N * ch.count * K * 2) + (size_t)N * ch.count * K * C) * sizeof(float);
}

extern "C" int kd_ocr_gather_fwd(const float *logits, int32_t ldl, const float *feats, int32_t ldf, float *ctx, float *mx, float *lse, int32_t N,
                                 int64_t HW, int32_t K, int32_t C, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    KD_REQUIRE(logits && feats && ctx && mx && lse && workspace && N > 0 && HW > 0 && HW < (1ll << 30) && K > 0 && C > 0 && ldl >= K && ldf >= C,
               KD_ERR_INVALID, "kd_ocr_gather_fwd: bad argument");
    KD_REQUIRE(K <= OCR_MAX_K && C % 4 == 0 && ok4(feats, ldf) && kd_aligned16(ctx) && kd_aligned16(workspace), KD_ERR_UNSUPPORTED,
               "kd_ocr_gather_fwd: K <= 32, C %% 4 == 0 and 16-byte aligned feats / ctx required");
    KD_REQUIRE(workspace_bytes >= kd_ocr_gather_workspace(N, HW, K, C), KD_ERR_WORKSPACE, "kd_ocr_gather_fwd: workspace too small");
    const Chunks ch = ocr_chunks(HW);
    float2 *stat = (float2 *)workspace;
    float *part = (float *)workspace + pad4((size_t)N * ch.count * K * 2);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ocr_stats_kernel, dim3(ch.count, N), dim3(256), 0, s, logits, ldl, stat, (int)HW, K, ch.per);
    hipLaunchKernelGGL(ocr_stats_finish_kernel, dim3(N), dim3(64), 0, s, stat, mx, lse, K, ch.count);
    hipLaunchKernelGGL(ocr_contract_kernel<true>, dim3(ch.count, (C + 255) / 256, N), dim3(256), 0, s, logits, ldl, lse, feats, ldf, part, (int)HW, K, C, ch.per);
    hipLaunchKernelGGL(ocr_contract_finish_kernel, dim3((unsigned)(((long long)N * K * (C / 4) + 255) / 256)), dim3(256), 0, s, part, ctx, N, K, C, ch.count);
    KD_CHECK_LAUNCH("kd_ocr_gather_fwd");
    return KD_OK;
}

extern "C" int kd_ocr_gather_bwd(const float *gctx, const float *ctx, const float *logits, int32_t ldl, const float *feats, int32_t ldf,
                                 const float *lse, float *d_feats, int32_t lddf, float *d_logits, int32_t lddl, int32_t N, int64_t HW, int32_t K,
                                 int32_t C, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    KD_REQUIRE(gctx && ctx && logits && feats && lse && d_feats && d_logits && workspace && N > 0 && HW > 0 && HW < (1ll << 30) && K > 0 && C > 0 &&
                   ldl >= K && lddl >= K && ldf >= C && lddf >= C, KD_ERR_INVALID, "kd_ocr_gather_bwd: bad argument");
    KD_REQUIRE(K <= OCR_MAX_K && C % 4 == 0 && ok4(feats, ldf) && ok4(d_feats, lddf) && kd_aligned16(gctx) && kd_aligned16(ctx), KD_ERR_UNSUPPORTED,
               "kd_ocr_gather_bwd: K <= 32, C %% 4 == 0 and 16-byte aligned views required");
    KD_REQUIRE((size_t)K * C * sizeof(float) <= OCR_LDS_LIMIT, KD_ERR_UNSUPPORTED, "kd_ocr_gather_bwd: the K x C context gradient must fit 64 KiB of LDS");
    KD_REQUIRE(workspace_bytes >= kd_ocr_gather_workspace(N, HW, K, C), KD_ERR_WORKSPACE, "kd_ocr_gather_bwd: workspace too small");
    float *dk = (float *)workspace;
    hipStream_t s = (hipStream_t)stream;
    const int per = ocr_pixels_per_block(HW);
    hipLaunchKernelGGL(ocr_rowdot_kernel, dim3(N * K), dim3(64), 0, s, gctx, ctx, dk, C);
    hipLaunchKernelGGL(ocr_gather_bwd_kernel, dim3((unsigned)((HW + per - 1) / per), N), dim3(256), (size_t)K * C * sizeof(float), s, gctx, dk, logits, ldl,
                       feats, ldf, lse, d_feats, lddf, d_logits, lddl, (int)HW, K, C, per);
    KD_CHECK_LAUNCH("kd_ocr_gather_bwd");
    return KD_OK;
}

extern "C" size_t kd_ocr_attend_workspace(int32_t N, int64_t HW, int32_t K, int32_t Ck)
{
    const Chunks ch = ocr_chunks(HW);
    // p | ds (N, HW, K each) | key-gradient partials | value-gradient partials (N, chunks, K, Ck each)
    return (2 * pad4((size_t)N * HW * K) + 2 * (size_t)N * ch.count * K * Ck) * sizeof(float);
}

static int attend_check(const char *who, const void *q, int ldq, const void *key, const void *value, const void *out, int ldo, int N, int64_t HW,
                        int K, int Ck)
{
    KD_REQUIRE(q && key && value && out && N > 0 && HW > 0 && HW < (1ll << 30) && K > 0 && Ck > 0 && ldq >= Ck && ldo >= Ck, KD_ERR_INVALID,
               "%s: bad argument", who);
    KD_REQUIRE(K <= OCR_MAX_K && Ck % 4 == 0 && ok4(q, ldq) && ok4(out, ldo) && kd_aligned16(key) && kd_aligned16(value), KD_ERR_UNSUPPORTED,
               "%s: K <= 32, Ck %% 4 == 0 and 16-byte aligned views required", who);
    KD_REQUIRE(2 * (size_t)K * Ck * sizeof(float) <= OCR_LDS_LIMIT, KD_ERR_UNSUPPORTED, "%s: the key and value panels must fit 64 KiB of LDS", who);
    return KD_OK;
}

extern "C" int kd_ocr_attend_fwd(const float *query, int32_t ldq, const float *key, const float *value, float *ctx, int32_t ldc, int32_t N, int64_t HW,
                                 int32_t K, int32_t Ck, float scale, kd_stream_t stream)
{
    const int rc = attend_check("kd_ocr_attend_fwd", query, ldq, key, value, ctx, ldc, N, HW, K, Ck);
    if (rc != KD_OK) return rc;
    const int per = ocr_pixels_per_block(HW);
    hipLaunchKernelGGL(ocr_attend_kernel<false>, dim3((unsigned)((HW + per - 1) / per), N), dim3(256), 2 * (size_t)K * Ck * sizeof(float), (hipStream_t)stream,
                       query, ldq, key, value, ctx, ldc, (const float *)nullptr, 0, (float *)nullptr, (float *)nullptr, (int)HW, K, Ck, scale, per);
    KD_CHECK_LAUNCH("kd_ocr_attend_fwd");
    return KD_OK;
}

extern "C" int kd_ocr_attend_bwd(const float *g, int32_t ldg, const float *query, int32_t ldq, const float *key, const float *value, float *d_query,
                                 int32_t lddq, float *d_key, float *d_value, int32_t N, int64_t HW, int32_t K, int32_t Ck, float scale, void *workspace,
                                 size_t workspace_bytes, kd_stream_t stream)
{
    const int rc = attend_check("kd_ocr_attend_bwd", query, ldq, key, value, d_query, lddq, N, HW, K, Ck);
    if (rc != KD_OK) return rc;
    KD_REQUIRE(g && d_key && d_value && workspace && ldg >= Ck, KD_ERR_INVALID, "kd_ocr_attend_bwd: bad argument");
    KD_REQUIRE(ok4(g, ldg) && kd_aligned16(d_key) && kd_aligned16(d_value) && kd_aligned16(workspace), KD_ERR_UNSUPPORTED,
               "kd_ocr_attend_bwd: 16-byte aligned views required");
    KD_REQUIRE(workspace_bytes >= kd_ocr_attend_workspace(N, HW, K, Ck), KD_ERR_WORKSPACE, "kd_ocr_attend_bwd: workspace too small");
    const Chunks ch = ocr_chunks(HW);
    float *wp = (float *)workspace, *wds = wp + pad4((size_t)N * HW * K);
    float *pk = wds + pad4((size_t)N * HW * K), *pv = pk + (size_t)N * ch.count * K * Ck;
    hipStream_t s = (hipStream_t)stream;
    const int per = ocr_pixels_per_block(HW);
    hipLaunchKernelGGL(ocr_attend_kernel<true>, dim3((unsigned)((HW + per - 1) / per), N), dim3(256), 2 * (size_t)K * Ck * sizeof(float), s, query, ldq, key,
                       value, d_query, lddq, g, ldg, wp, wds, (int)HW, K, Ck, scale, per);
    const dim3 gc(ch.count, (Ck + 255) / 256, N);
    const unsigned gf = (unsigned)(((long long)N * K * (Ck / 4) + 255) / 256);
    hipLaunchKernelGGL(ocr_contract_kernel<false>, gc, dim3(256), 0, s, wds, K, (const float *)nullptr, query, ldq, pk, (int)HW, K, Ck, ch.per);
    hipLaunchKernelGGL(ocr_contract_finish_kernel, dim3(gf), dim3(256), 0, s, pk, d_key, N, K, Ck, ch.count);
    hipLaunchKernelGGL(ocr_contract_kernel<false>, gc, dim3(256), 0, s, wp, K, (const float *)nullptr, g, ldg, pv, (int)HW, K, Ck, ch.per);
    hipLaunchKernelGGL(ocr_contract_finish_kernel, dim3(gf), dim3(256), 0, s, pv, d_value, N, K, Ck, ch.count);
    KD_CHECK_LAUNCH("kd_ocr_attend_bwd");
    return KD_OK;
}
