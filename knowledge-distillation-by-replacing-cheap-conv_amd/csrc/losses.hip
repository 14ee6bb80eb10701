// KD losses, forward + gradient fused in one pass (kd_kldiv, kd_hint_mse,
// kd_weighted_hint_mse, kd_ce2d, kd_jsdiv, kd_ensemble_kldiv, kd_focal, kd_topk_hint_mse, kd_kldiv_multi),
// the ensemble's mean softmax (kd_softmax_mean) and the RAdam update (kd_radam_step).
// All are HBM-bound streaming kernels.  Loss scalars are reduced in two fixed-order
// stages (per-block partials in fp64 -> one finishing block), so results are
// bit-reproducible run to run.
#include <algorithm>
#include <type_traits>

#include "kd_common.h"
#include "loss_select.h"

namespace {

// K per-thread sums -> out[q][blockIdx.x], q < K: a wave reduction, then the four waves added in a fixed order
template <int K> __device__ __forceinline__ void block_partials(const double (&v)[K], double *const (&out)[K])
{
    __shared__ double w[K][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < K; ++q) {
        const double s = wave_sum_d(v[q]);
        if (lane == 0) w[q][wv] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < K; ++q) out[q][blockIdx.x] = w[q][0] + w[q][1] + w[q][2] + w[q][3];
    }
}

// loss = scale * sum(partial[0..n)) / (denom_ptr ? sum(partial2) : 1)
__global__ __launch_bounds__(256) void finish_kernel(const double *partial, int n, double scale, const double *count,
                                                     float *loss)
{
    __shared__ double sh[256], sc[256];
    double s = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) { s += partial[i]; if (count) c += count[i]; }
    sh[threadIdx.x] = s; sc[threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { sh[threadIdx.x] += sh[threadIdx.x + o]; sc[threadIdx.x] += sc[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double v = sh[0] * scale;
        if (count) v = sc[0] > 0.0 ? v / sc[0] : 0.0;
        *loss = (float)v;
    }
}

struct V3 { const void *p; int dt; long long sN, sC, sP; };
struct M3 { void *p; int dt; long long sN, sC, sP; };

// ---- confusion matrix (logged mIoU): argmax over channels + C x C histogram ------------------------------------------
// Integer work, so the result is exact whatever the order: per-block histogram in LDS (integer atomics), flushed with
// 64-bit integer atomics.  argmax = first index of the maximum (torch.argmax), a NaN counts as the maximum.
__device__ __forceinline__ bool arg_better(float a, float m) { return a > m || (a != a && m == m); }

template <typename TX>
__global__ __launch_bounds__(256) void confusion_nhwc_kernel(const TX *__restrict__ x, const int64_t *__restrict__ target, int C,
                                                             long long npix, unsigned long long *conf)
{
    extern __shared__ float sm[];              // 256 pixels x C logits, then C*C counters
    unsigned int *hist = (unsigned int *)(sm + 256 * C);
    for (int i = threadIdx.x; i < C * C; i += 256) hist[i] = 0u;
    __syncthreads();
    for (long long base = (long long)blockIdx.x * 256; base < npix; base += (long long)gridDim.x * 256) {
        const int np = (int)min((long long)256, npix - base);
        const int nel = np * C;
        const TX *xp = x + base * C;
        for (int i = threadIdx.x; i < nel; i += 256) sm[i] = Elem<TX>::ld(xp + i);
        __syncthreads();
        if ((int)threadIdx.x < np) {
            const int64_t y = target[base + threadIdx.x];
            if (y >= 0 && y < C) {
                const float *a = sm + threadIdx.x * C;
                float m = a[0];
                int am = 0;
                for (int c = 1; c < C; ++c)
                    if (arg_better(a[c], m)) { m = a[c]; am = c; }
                atomicAdd(&hist[(int)y * C + am], 1u);
            }
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < C * C; i += 256)
        if (hist[i]) atomicAdd(&conf[i], (unsigned long long)hist[i]);
}

__global__ __launch_bounds__(256) void confusion_kernel(V3 x, const int64_t *__restrict__ target, int N, int C, long long P,
                                                        unsigned long long *conf)
{
    extern __shared__ float sm[];
    unsigned int *hist = (unsigned int *)sm;
    for (int i = threadIdx.x; i < C * C; i += 256) hist[i] = 0u;
    __syncthreads();
    const long long total = (long long)N * P;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int64_t y = target[i];
        if (y < 0 || y >= C) continue;
        const long long n = i / P, p = i - n * P;
        const long long b = n * x.sN + p * x.sP;
        float m = kd_ld(x.p, x.dt, b);
        int am = 0;
        for (int c = 1; c < C; ++c) {
            const float a = kd_ld(x.p, x.dt, b + c * x.sC);
            if (arg_better(a, m)) { m = a; am = c; }
        }
        atomicAdd(&hist[(int)y * C + am], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += 256)
        if (hist[i]) atomicAdd(&conf[i], (unsigned long long)hist[i]);
}

// ---- global <-> LDS staging of the NHWC-dense fast paths ------------------------------------------------------------
// global -> LDS staging of `nel` consecutive elements (scaled): 16-B vectors when the operand is fp32, the chunk is whole and
// 16-B aligned (19 scalar loads per thread and operand otherwise: the 19-class logit kernels ran at 2.5 TB/s)
template <typename T> __device__ __forceinline__ void stage_scaled(float *dst, const T *src, int nel, float mul)
{
    if (std::is_same<T, float>::value && (nel & 3) == 0 && ((uintptr_t)src & 15) == 0) {
        const float4 *s4 = (const float4 *)src;
        float4 *d4 = (float4 *)dst;
        for (int i = threadIdx.x; i < (nel >> 2); i += 256) {
            float4 v = s4[i];
            v.x *= mul; v.y *= mul; v.z *= mul; v.w *= mul;
            d4[i] = v;
        }
    } else {
        for (int i = threadIdx.x; i < nel; i += 256) dst[i] = Elem<T>::ld(src + i) * mul;
    }
}
template <typename T> __device__ __forceinline__ void unstage(T *dst, const float *src, int nel)
{
    if (std::is_same<T, float>::value && (nel & 3) == 0 && ((uintptr_t)dst & 15) == 0) {
        const float4 *s4 = (const float4 *)src;
        float4 *d4 = (float4 *)dst;
        for (int i = threadIdx.x; i < (nel >> 2); i += 256) d4[i] = s4[i];
    } else {
        for (int i = threadIdx.x; i < nel; i += 256) Elem<T>::st(dst + i, src[i]);
    }
}

template <typename TX>
__global__ __launch_bounds__(256) void ce2d_nhwc_kernel(const TX *__restrict__ x, const int64_t *__restrict__ target, int ignore_index,
                                                        int C, long long npix, double *partial, double *count, const float *__restrict__ cw)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    double acc = 0.0, cnt = 0.0;
    for (long long base = (long long)blockIdx.x * 256; base < npix; base += (long long)gridDim.x * 256) {
        const int np = (int)min((long long)256, npix - base);
        const int nel = np * C;
        const TX *xp = x + base * C;
        stage_scaled(sm, xp, nel, 1.0f);
        __syncthreads();
        if ((int)threadIdx.x < np) {
            const int64_t y = target[base + threadIdx.x];
            if (!(y == ignore_index || y < 0 || y >= C)) {
                const float *a = sm + threadIdx.x * C;
                float m = -INFINITY;
                for (int c = 0; c < C; ++c) m = fmaxf(m, a[c]);
                float z = 0.f;
                for (int c = 0; c < C; ++c) z += __expf(a[c] - m);
                const float wy = cw ? cw[y] : 1.f;      // (class weights: nn.NLLLoss(weight): sum_i w[y_i] * nll_i / sum_i w[y_i])
                acc += (double)(wy * -(a[y] - m - __logf(z)));
                cnt += (double)wy;
            }
        }
        __syncthreads();
    }
    __shared__ double w1[4], w2[4];
    acc = wave_sum_d(acc); cnt = wave_sum_d(cnt);
    if ((threadIdx.x & 63) == 0) { w1[threadIdx.x >> 6] = acc; w2[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) { partial[blockIdx.x] = w1[0] + w1[1] + w1[2] + w1[3]; count[blockIdx.x] = w2[0] + w2[1] + w2[2] + w2[3]; }
}

// ---- logit losses straight from the LOW-RESOLUTION logits ---------------------------------------------------------------------------
// The decoder's classifier produces (N,h,w,C) fp32 logits; the reference up-samples them bilinearly to the input size
// (models/deeplabv3/deeplabv3.py:160-162) and the trainer logs CE(student), CE(teacher) and KLDiv on the full-resolution tensors
// (trainer/layerwise_trainer.py:222-227).  Materialised, that is two 1.27-GB fp32 tensors per 8 images written once and read back by
// three kernels (2.3 ms per step).  Here a pixel's C logits are interpolated in registers -- the horizontal blend of each
// source row, then the vertical blend -- from a low-resolution patch staged in LDS: a
// workgroup takes 256 consecutive output pixels of one output row, i.e. <= UP_NW source columns of two source rows.
constexpr int UP_NW = LOSS_UP_NW;   // one value: the header refuses what would not fit, the kernels size their staged patch by it

struct UpGeom { int N, h, w, C, H, W; float sh, sw, oh, ow; };

// stage rows h0 / h1, columns [wlo, wlo + nw) of image n: 2 * nw * C contiguous floats per row
__device__ __forceinline__ void up_stage(float *sm, const float *__restrict__ x, const UpGeom &g, int n, int h0, int h1, int wlo, int nw)
{
    const int nel = nw * g.C;
    const float *r0 = x + (((size_t)n * g.h + h0) * g.w + wlo) * g.C, *r1 = x + (((size_t)n * g.h + h1) * g.w + wlo) * g.C;
    // loads in batches of 8 per row, all in flight together (one load -> one LDS store per iteration waits a memory latency per
    // iteration: 10+ us per chunk)
    for (int base = threadIdx.x; base < nel; base += 8 * 256) {
        float a[8], b[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = base + k * 256;
            a[k] = i < nel ? r0[i] : 0.f;
            b[k] = i < nel ? r1[i] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = base + k * 256;
            if (i < nel) { sm[i] = a[k]; sm[nel + i] = b[k]; }
        }
    }
}
__device__ __forceinline__ float up_val(const float *sm, int nelrow, int o0, int o1, int c, float aw, float ah)
{
    const float l0 = resample_lerp(aw, sm[o0 + c], sm[o1 + c]);
    const float l1 = resample_lerp(aw, sm[nelrow + o0 + c], sm[nelrow + o1 + c]);
    return resample_lerp(ah, l0, l1);
}
// chunk -> (n, ho, first output column); source rows / columns of the chunk
struct UpChunk { int n, ho, wo0, h0, h1, wlo, nw; float ah; };
__device__ __forceinline__ UpChunk up_chunk(const UpGeom &g, long long chunk, int cpr)
{
    UpChunk k;
    const long long row = chunk / cpr;
    k.wo0 = (int)(chunk - row * cpr) * 256;
    k.n = (int)(row / g.H);
    k.ho = (int)(row - (long long)k.n * g.H);
    resample_src(k.ho, g.sh, g.oh, g.h, k.h0, k.h1, k.ah);
    // the staged columns: the first source column of the chunk's first output column to the second of its last
    int a, b, unused; float f;
    resample_src(k.wo0, g.sw, g.ow, g.w, a, unused, f);
    resample_src(min(k.wo0 + 255, g.W - 1), g.sw, g.ow, g.w, unused, b, f);
    k.wlo = a; k.nw = b - a + 1;
    return k;
}
// output column wo of a chunk: its horizontal blend weight, the offsets of its two source columns in a staged row, the row length
struct UpCol { float aw; int o0, o1, nr; };
__device__ __forceinline__ UpCol up_col(const UpGeom &g, const UpChunk &k, int wo)
{
    int w0, w1; float aw;
    resample_src(wo, g.sw, g.ow, g.w, w0, w1, aw);
    return UpCol{aw, (w0 - k.wlo) * g.C, (w1 - k.wlo) * g.C, k.nw * g.C};
}
// One interpolated pixel of a staged patch, channel c through operator().  CT: the class count at compile time (19: the logits
// are interpolated ONCE into registers) or 0 (any C: re-interpolated at every read).  mul: the 1/T of the two-distribution losses.
template <int CT> struct UpPix {
    const float *sm;
    UpCol col;
    float ah, mul, v[CT > 0 ? CT : 1];
    __device__ __forceinline__ UpPix(const float *sm_, const UpCol &col_, float ah_, float mul_ = 1.f) : sm(sm_), col(col_), ah(ah_), mul(mul_)
    {
        if constexpr (CT > 0) {
#pragma unroll
            for (int c = 0; c < CT; ++c) v[c] = up_val(sm, col.nr, col.o0, col.o1, c, col.aw, ah) * mul;
        }
    }
    __device__ __forceinline__ float operator()(int c) const
    {
        if constexpr (CT > 0) return v[c];
        else return up_val(sm, col.nr, col.o0, col.o1, c, col.aw, ah) * mul;
    }
    // channel y, known at run time only (a select per register, never an indexed register array)
    __device__ __forceinline__ float at(int y) const
    {
        if constexpr (CT > 0) {
            float r = 0.f;
#pragma unroll
            for (int c = 0; c < CT; ++c) r = c == y ? v[c] : r;
            return r;
        } else {
            return (*this)(y);
        }
    }
};

template <int CT>
__global__ __launch_bounds__(256) void ce2d_up_kernel(const float *__restrict__ x, const int64_t *__restrict__ target, int ignore_index,
                                                      UpGeom g, long long nchunks, int cpr, double *partial, double *count)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int C = CT > 0 ? CT : g.C;
    constexpr int UR = CT > 0 ? CT : 8;   // (fully unrolled at a compile-time class count, 8-way at any other)
    double acc = 0.0, cnt = 0.0;
    for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const UpChunk k = up_chunk(g, chunk, cpr);
        up_stage(sm, x, g, k.n, k.h0, k.h1, k.wlo, k.nw);
        __syncthreads();
        const int wo = k.wo0 + threadIdx.x;
        if (wo < g.W) {
            const int64_t y = target[((size_t)k.n * g.H + k.ho) * g.W + wo];
            if (!(y == ignore_index || y < 0 || y >= g.C)) {
                const UpPix<CT> v(sm, up_col(g, k, wo), k.ah);
                float m = -INFINITY, z = 0.f;
                // (no count on the max pass: a compile-time C unrolls fully by itself, a run-time C as the compiler chooses)
                for (int c = 0; c < C; ++c) m = fmaxf(m, v(c));
#pragma unroll UR
                for (int c = 0; c < C; ++c) z += __expf(v(c) - m);
                acc += (double)(-(v.at((int)y) - m - __logf(z)));
                cnt += 1.0;
            }
        }
        __syncthreads();
    }
    block_partials<2>({acc, cnt}, {partial, count});
}

// ---- the analysis step's logged metrics from both low-resolution logit tensors (trainer/analysis_trainer.py:55-81) ---------------------
// One pass: CE(student), CE(teacher), sum (s - t)^2 and both confusion matrices (argmax = first maximum, as confusion_nhwc_kernel).
// Partials: [ce_s | ce_t | count | sq] x MET_MAX_BLOCKS doubles inside kd_loss_workspace's 2 * LOSS_MAX_BLOCKS; the histograms are LDS
// integer atomics flushed once per block (exact in any order).
constexpr int MET_MAX_BLOCKS = LOSS_MET_MAX_BLOCKS;   // one value: the header caps the grid, the kernels stride their partial arrays by it

template <int CT>
__global__ __launch_bounds__(256) void logit_metrics_up_kernel(const float *__restrict__ s, const float *__restrict__ t,
                                                               const int64_t *__restrict__ target, int ignore_index, UpGeom g,
                                                               long long nchunks, int cpr, double *partial,
                                                               unsigned long long *conf_s, unsigned long long *conf_t)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *ss = sm, *st = sm + 2 * UP_NW * g.C;
    unsigned int *hs = (unsigned int *)(sm + 4 * UP_NW * g.C), *ht = hs + g.C * g.C;
    for (int i = threadIdx.x; i < 2 * g.C * g.C; i += 256) hs[i] = 0u;
    const int C = CT > 0 ? CT : g.C;
    constexpr int UR = CT > 0 ? CT : 2;   // (two operands and two histograms a pixel: 2-way at a run-time class count)
    double ces = 0.0, cet = 0.0, cnt = 0.0, sq = 0.0;
    for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const UpChunk k = up_chunk(g, chunk, cpr);
        up_stage(ss, s, g, k.n, k.h0, k.h1, k.wlo, k.nw);
        up_stage(st, t, g, k.n, k.h0, k.h1, k.wlo, k.nw);
        __syncthreads();
        const int wo = k.wo0 + threadIdx.x;
        if (wo < g.W) {
            const int64_t y = target[((size_t)k.n * g.H + k.ho) * g.W + wo];
            const bool lab = y >= 0 && y < g.C;                    // counted by the confusion matrices (kd_confusion)
            const bool valid = lab && y != ignore_index;           // counted by the cross entropies (kd_ce2d)
            const int yc = lab ? (int)y : 0;
            const UpCol col = up_col(g, k, wo);
            const UpPix<CT> a(ss, col, k.ah), b(st, col, k.ah);
            float ms = a(0), mt = b(0), zs = 0.f, zt = 0.f, d2 = 0.f;
            int as = 0, at = 0;
#pragma unroll UR
            for (int c = 0; c < C; ++c) {
                const float av = a(c), bv = b(c);
                if (c > 0 && arg_better(av, ms)) { ms = av; as = c; }
                if (c > 0 && arg_better(bv, mt)) { mt = bv; at = c; }
                const float d = av - bv;
                d2 += d * d;
            }
#pragma unroll UR
            for (int c = 0; c < C; ++c) { zs += __expf(a(c) - ms); zt += __expf(b(c) - mt); }
            const float vs = a.at(yc), vt = b.at(yc);
            sq += (double)d2;
            if (valid) {
                ces += (double)(-(vs - ms - __logf(zs)));
                cet += (double)(-(vt - mt - __logf(zt)));
                cnt += 1.0;
            }
            if (lab) {
                atomicAdd(&hs[yc * g.C + as], 1u);
                atomicAdd(&ht[yc * g.C + at], 1u);
            }
        }
        __syncthreads();
    }
    __shared__ double wsum[4][4];
    ces = wave_sum_d(ces); cet = wave_sum_d(cet); cnt = wave_sum_d(cnt); sq = wave_sum_d(sq);
    if ((threadIdx.x & 63) == 0) {
        double *r = wsum[threadIdx.x >> 6];
        r[0] = ces; r[1] = cet; r[2] = cnt; r[3] = sq;
    }
    __syncthreads();
    if (threadIdx.x < 4)
        partial[threadIdx.x * MET_MAX_BLOCKS + blockIdx.x] = wsum[0][threadIdx.x] + wsum[1][threadIdx.x] + wsum[2][threadIdx.x] + wsum[3][threadIdx.x];
    for (int i = threadIdx.x; i < g.C * g.C; i += 256) {
        if (hs[i]) atomicAdd(&conf_s[i], (unsigned long long)hs[i]);
        if (ht[i]) atomicAdd(&conf_t[i], (unsigned long long)ht[i]);
    }
}

// out[0] = CE(student), out[1] = CE(teacher) (0 when no pixel is valid, like finish_kernel), out[2] = sum sq / numel
__global__ __launch_bounds__(256) void logit_metrics_finish_kernel(const double *partial, int n, double inv_numel, float *out)
{
    __shared__ double sh[4][256];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += 256)
        for (int q = 0; q < 4; ++q) v[q] += partial[q * MET_MAX_BLOCKS + i];
    for (int q = 0; q < 4; ++q) sh[q][threadIdx.x] = v[q];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o)
            for (int q = 0; q < 4; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double c = sh[2][0];
        out[0] = (float)(c > 0.0 ? sh[0][0] / c : 0.0);
        out[1] = (float)(c > 0.0 ? sh[1][0] / c : 0.0);
        out[2] = (float)(sh[3][0] * inv_numel);
    }
}

// ---- hint MSE -----------------------------------------------------------------------------
// contiguous fast path: s, t, g share one dense layout -> 8 elements per thread per step
template <typename T>
__global__ __launch_bounds__(256) void mse_vec_kernel(const T *__restrict__ s, const T *__restrict__ t, T *__restrict__ g,
                                                      float gscale, long long n8, double *partial)
{
    float acc = 0.f;
    double dacc = 0.0;
    int cnt = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        float a[8], b[8], d[8];
        ld8(s + i * 8, a);
        ld8(t + i * 8, b);
#pragma unroll
        for (int q = 0; q < 8; ++q) { d[q] = a[q] - b[q]; acc = fmaf(d[q], d[q], acc); }
        if (g) {
#pragma unroll
            for (int q = 0; q < 8; ++q) d[q] *= gscale;
            st8(g + i * 8, d);
        }
        if (++cnt == 16) { dacc += (double)acc; acc = 0.f; cnt = 0; }  // bound fp32 accumulation length
    }
    dacc += (double)acc;
    block_partials<1>({dacc}, {partial});
}
__global__ __launch_bounds__(256) void mse_strided_kernel(V3 s, V3 t, M3 g, float gscale, int N, int C, long long P,
                                                          int c_fast, double *partial)
{
    double acc = 0.0;
    const long long total = (long long)N * C * P;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long n, c, p;
        if (c_fast) { c = i % C; const long long r = i / C; p = r % P; n = r / P; }
        else { p = i % P; const long long r = i / P; c = r % C; n = r / C; }
        const float d = kd_ld(s.p, s.dt, n * s.sN + c * s.sC + p * s.sP) - kd_ld(t.p, t.dt, n * t.sN + c * t.sC + p * t.sP);
        acc += (double)d * d;
        if (g.p) kd_st(g.p, g.dt, n * g.sN + c * g.sC + p * g.sP, gscale * d);
    }
    block_partials<1>({acc}, {partial});
}

// ---- weighted hint MSE ---------------------------------------------------------------------
__global__ void wsum_kernel(const float *w, int per_sample, int N, int C, float *wsum)
{
    // one wave per sample
    const int n = blockIdx.x, lane = threadIdx.x;
    const float *wn = w + (per_sample ? (size_t)n * C : 0);
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += wn[c];
    s = wave_sum(s);
    if (lane == 0) wsum[n] = s;
}
// grid: x = P chunks, y = ceil(C/256), z = N ; thread = one channel, loops over its pixel chunk
__global__ __launch_bounds__(256) void whmse_kernel(V3 s, V3 t, M3 g, const float *w, int per_sample, const float *wsum,
                                                    float gscale, int N, int C, long long P, long long per_chunk,
                                                    double *partial)
{
    const int c = blockIdx.y * 256 + threadIdx.x, n = blockIdx.z;
    double contrib = 0.0;
    if (c < C) {
        const float wc = w[(per_sample ? (size_t)n * C : 0) + c], ws = wsum[n];
        const float gs = gscale * wc / (ws * (float)N * (float)P) * 2.f;
        const long long p0 = blockIdx.x * per_chunk, p1 = min(P, p0 + per_chunk);
        float acc = 0.f;
        for (long long p = p0; p < p1; ++p) {
            const float d = kd_ld(s.p, s.dt, n * s.sN + c * s.sC + p * s.sP) - kd_ld(t.p, t.dt, n * t.sN + c * t.sC + p * t.sP);
            acc = fmaf(d, d, acc);
            if (g.p) kd_st(g.p, g.dt, n * g.sN + c * g.sC + p * g.sP, gs * d);
        }
        contrib = (double)acc * (double)wc / ((double)ws * (double)P);
    }
    // block partial, flattened block index
    __shared__ double wsm[4];
    contrib = wave_sum_d(contrib);
    if ((threadIdx.x & 63) == 0) wsm[threadIdx.x >> 6] = contrib;
    __syncthreads();
    if (threadIdx.x == 0)
        partial[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = wsm[0] + wsm[1] + wsm[2] + wsm[3];
}

// ---- cross entropy (logged metric) ----------------------------------------------------------
__global__ __launch_bounds__(256) void ce2d_kernel(V3 x, const int64_t *target, int ignore_index, int N, int C, long long P,
                                                   double *partial, double *count, const float *cw)
{
    double acc = 0.0, cnt = 0.0;
    const long long total = (long long)N * P;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int64_t y = target[i];
        if (y == ignore_index || y < 0 || y >= C) continue;
        const long long n = i / P, p = i - n * P;
        const long long b = n * x.sN + p * x.sP;
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) m = fmaxf(m, kd_ld(x.p, x.dt, b + c * x.sC));
        float z = 0.f;
        for (int c = 0; c < C; ++c) z += __expf(kd_ld(x.p, x.dt, b + c * x.sC) - m);
        const float wy = cw ? cw[y] : 1.f;
        acc += (double)(wy * -(kd_ld(x.p, x.dt, b + y * x.sC) - m - __logf(z)));
        cnt += (double)wy;
    }
    __shared__ double w1[4], w2[4];
    acc = wave_sum_d(acc); cnt = wave_sum_d(cnt);
    if ((threadIdx.x & 63) == 0) { w1[threadIdx.x >> 6] = acc; w2[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) { partial[blockIdx.x] = w1[0] + w1[1] + w1[2] + w1[3]; count[blockIdx.x] = w2[0] + w2[1] + w2[2] + w2[3]; }
}

// gradient of the cross entropy above: (softmax - onehot) / #valid, zero rows for ignored pixels.  count[] holds the forward's
// per-block valid-pixel counts (any block count nb); every block sums them in the same order.
__global__ __launch_bounds__(256) void ce2d_count_kernel(const int64_t *target, int ignore_index, int C, long long total, double *count, const float *cw)
{
    double cnt = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int64_t y = target[i];
        if (!(y == ignore_index || y < 0 || y >= C)) cnt += cw ? (double)cw[y] : 1.0;
    }
    __shared__ double w2[4];
    cnt = wave_sum_d(cnt);
    if ((threadIdx.x & 63) == 0) w2[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) count[blockIdx.x] = w2[0] + w2[1] + w2[2] + w2[3];
}

__global__ __launch_bounds__(256) void ce2d_grad_kernel(V3 x, const int64_t *target, int ignore_index, int N, int C, long long P, M3 g,
                                                        float gscale, const double *count, int ncount, const float *cw, int sum_reduction)
{
    __shared__ double tot;
    if (threadIdx.x == 0) {
        double c = 0.0;
        for (int i = 0; i < ncount; ++i) c += count[i];
        tot = c;
    }
    __syncthreads();
    const float k = sum_reduction ? gscale : (tot > 0.0 ? gscale / (float)tot : 0.f);
    const long long total = (long long)N * P;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int64_t y = target[i];
        const long long n = i / P, p = i - n * P;
        const long long b = n * x.sN + p * x.sP, gb = n * g.sN + p * g.sP;
        if (y == ignore_index || y < 0 || y >= C) {
            for (int c = 0; c < C; ++c) kd_st(g.p, g.dt, gb + c * g.sC, 0.f);
            continue;
        }
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) m = fmaxf(m, kd_ld(x.p, x.dt, b + c * x.sC));
        float z = 0.f;
        for (int c = 0; c < C; ++c) z += __expf(kd_ld(x.p, x.dt, b + c * x.sC) - m);
        const float iz = 1.f / z, kw = cw ? k * cw[y] : k;
        for (int c = 0; c < C; ++c) {
            const float pr = __expf(kd_ld(x.p, x.dt, b + c * x.sC) - m) * iz;
            kd_st(g.p, g.dt, gb + c * g.sC, kw * (pr - (c == (int)y ? 1.f : 0.f)));
        }
    }
}

// ---- RAdam ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void radam_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                    float *__restrict__ v, long long n, float beta1, float beta2, float eps,
                                                    float wd_lr, float step_lr, int rectified)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float gi = g[i];
        const float vi = v[i] * beta2 + (1.f - beta2) * gi * gi;
        const float mi = m[i] * beta1 + (1.f - beta1) * gi;
        v[i] = vi; m[i] = mi;
        float pi = p[i];
        if (wd_lr != 0.f) pi += -wd_lr * pi;
        pi += rectified ? -step_lr * mi / (sqrtf(vi) + eps) : -step_lr * mi;
        p[i] = pi;
    }
}

// Multi-tensor form: one launch updates up to RADAM_MAXT tensors.  The per-tensor constants travel by value in the kernel
// argument (no device-side table to fill, hence no copy and no sync); a block finds its tensor by a short search in the
// block-prefix table.  Element-wise arithmetic identical to radam_kernel.
constexpr int RADAM_MAXT = 48;
constexpr int RADAM_BLK = 256 * 8;   // elements per block
struct RadamBatch {
    float *p[RADAM_MAXT];
    const float *g[RADAM_MAXT];
    float *m[RADAM_MAXT];
    float *v[RADAM_MAXT];
    long long n[RADAM_MAXT];
    int blk0[RADAM_MAXT + 1];        // first block of tensor t
    float wd_lr[RADAM_MAXT], step_lr[RADAM_MAXT], beta1[RADAM_MAXT], beta2[RADAM_MAXT], eps[RADAM_MAXT];
    int rect[RADAM_MAXT];
    int count;
};
static_assert(sizeof(RadamBatch) <= 4096, "kernel argument space");
__global__ __launch_bounds__(256) void radam_multi_kernel(const RadamBatch b)
{
    int lo = 0, hi = b.count - 1;
    while (lo < hi) {   // block-uniform
        const int mid = (lo + hi + 1) >> 1;
        if (b.blk0[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const int t = lo;
    float *__restrict__ p = b.p[t];
    const float *__restrict__ g = b.g[t];
    float *__restrict__ m = b.m[t];
    float *__restrict__ v = b.v[t];
    const float beta1 = b.beta1[t], beta2 = b.beta2[t], eps = b.eps[t], wd_lr = b.wd_lr[t], step_lr = b.step_lr[t];
    const int rectified = b.rect[t];
    const long long base = (long long)((int)blockIdx.x - b.blk0[t]) * RADAM_BLK;
    const long long end = min(b.n[t], base + RADAM_BLK);
    for (long long i = base + threadIdx.x; i < end; i += 256) {
        const float gi = g[i];
        const float vi = v[i] * beta2 + (1.f - beta2) * gi * gi;
        const float mi = m[i] * beta1 + (1.f - beta1) * gi;
        v[i] = vi; m[i] = mi;
        float pi = p[i];
        if (wd_lr != 0.f) pi += -wd_lr * pi;
        pi += rectified ? -step_lr * mi / (sqrtf(vi) + eps) : -step_lr * mi;
        p[i] = pi;
    }
}

inline V3 v3(const kd_view3 *v) { return V3{v->ptr, v->dtype, (long long)v->sN, (long long)v->sC, (long long)v->sP}; }
inline M3 m3(const kd_mview3 *v)
{
    if (!v) return M3{nullptr, 0, 0, 0, 0};
    return M3{v->ptr, v->dtype, (long long)v->sN, (long long)v->sC, (long long)v->sP};
}
inline bool ok_dt(int d) { return d == KD_F32 || d == KD_BF16; }

// ---- upstream-gradient scale of a fused loss gradient ---------------------------------------------------------------------
// autograd hands the loss Function d(total)/d(loss) as a device scalar; for `loss = sum of hint losses` (layerwise_trainer.py:
// 229-235) it is exactly 1 and grad * 1 is a full read + write of every hint-sized gradient for nothing.  The test is made on
// the device (no host sync): every thread reads the scalar and leaves when it is 1.
template <typename T>
__global__ __launch_bounds__(256) void scale_by_device_scalar_kernel(T *x, long long n8, long long n, const float *s)
{
    const float sv = *s;
    if (sv == 1.0f) return;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        float v[8];
        ld8(x + i * 8, v);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] *= sv;
        st8(x + i * 8, v);
    }
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)(n - n8 * 8)) {
        const long long i = n8 * 8 + threadIdx.x;
        Elem<T>::st(x + i, Elem<T>::ld(x + i) * sv);
    }
}

// ---- KLDiv / JSD / ensemble KL: the two-distribution criteria -----------------------------------------------------------------
// One pixel's C-vector through an accessor (LDS row, register array, strided global or in-register interpolation): ls(c) / lt(c)
// return the student / target value at channel c (already divided by T), sg(c, v) stores the gradient.  CT > 0: the class count
// at compile time (loops unrolled, register arrays stay registers).
//   PAIR_KLD (losses/KLDiv.py): value sum_c pt (lpt - lps); grad gscale * (ps - pt), stored in the value's own pass
//   PAIR_JSD (losses/JSDiv.py:19-26): value sum_c ps (lps - lq) + pt (lpt - lq), lq = log 1/2 + logaddexp(lps, lpt)
//                                      grad  gscale * ps * (a - <ps, a>), a = lps - lq
//   PAIR_EKL (losses/EnsembleKLDiv.py:17-21): t holds probabilities; value sum_c xlogy(t, t) - t lps
//                                      grad  gscale * (ps * sum_c t - t)
enum { PAIR_KLD = 0, PAIR_JSD = 1, PAIR_EKL = 2 };

__device__ __forceinline__ float log_half_sum(float x, float y)
{
    const float mx = fmaxf(x, y), mn = fminf(x, y);
    return -0.693147180559945309f + mx + log1pf(__expf(mn - mx));
}

// log q = log (ps + pt)/2: one hardware log while ps + pt is a normal number, log space (log 1/2 + logaddexp) below that
__device__ __forceinline__ float jsd_log_q(float lps, float lpt, float ps, float pt)
{
    const float sum = ps + pt;
    return sum > 1e-30f ? __logf(0.5f * sum) : log_half_sum(lps, lpt);
}

// STASH: the caller's rows are writable (LDS): the forward pass parks ps and a in them (put), the gradient pass reads them back
// (get) instead of recomputing two exponentials and a logarithm per element
// UR0: the unrolling of the loops at a run-time class count (CT == 0), the caller's choice: 8 where a read is an LDS access and the
// body short (the KL kernels over LDS), 1 (rolled) where it is a strided global load or the body long (JSD / EKL)
template <int KIND, int CT, bool STASH, int UR0, typename LS, typename LT, typename SG, typename PUT, typename GET>
__device__ __forceinline__ float pair_pixel(int C_, LS ls, LT lt, SG sg, PUT put, GET get, bool want_grad, float gscale)
{
    const int C = CT > 0 ? CT : C_;
    constexpr int UR = CT > 0 ? CT : UR0;
    constexpr bool TLOGITS = KIND != PAIR_EKL;   // the target holds logits too: its softmax statistics ride in the student's passes
    float ms = -INFINITY, mt = -INFINITY;
#pragma unroll UR
    for (int c = 0; c < C; ++c) {
        ms = fmaxf(ms, ls(c));
        if constexpr (TLOGITS) mt = fmaxf(mt, lt(c));
    }
    float zs = 0.f, zt = 0.f;
#pragma unroll UR
    for (int c = 0; c < C; ++c) {
        zs += __expf(ls(c) - ms);
        if constexpr (TLOGITS) zt += __expf(lt(c) - mt);
    }
    const float lzs = __logf(zs) + ms;
    [[maybe_unused]] const float lzt = __logf(zt) + mt;
    float val = 0.f;
    if constexpr (KIND == PAIR_KLD) {
        constexpr int URG = CT > 0 ? CT : (UR0 > 4 ? 4 : UR0);   // (this pass stores as well: at most 4-way at a run-time class count)
#pragma unroll URG
        for (int c = 0; c < C; ++c) {
            const float lps = ls(c) - lzs, lpt = lt(c) - lzt, pt = __expf(lpt);
            val += pt > 0.f ? pt * (lpt - lps) : 0.f;
            if (want_grad) sg(c, gscale * (__expf(lps) - pt));
        }
    } else if constexpr (KIND == PAIR_JSD) {
        float dot = 0.f;
#pragma unroll UR
        for (int c = 0; c < C; ++c) {
            const float lps = ls(c) - lzs, lpt = lt(c) - lzt, ps = __expf(lps), pt = __expf(lpt);
            const float lq = jsd_log_q(lps, lpt, ps, pt), a = lps - lq;
            const float psa = ps > 0.f ? ps * a : 0.f;
            val += psa + (pt > 0.f ? pt * (lpt - lq) : 0.f);
            dot += psa;
            if constexpr (STASH) put(c, ps, a);
        }
        if (want_grad) {
#pragma unroll UR
            for (int c = 0; c < C; ++c) {
                float ps, a;
                if constexpr (STASH) {
                    get(c, ps, a);
                } else {
                    const float lps = ls(c) - lzs, lpt = lt(c) - lzt, pt = __expf(lpt);
                    ps = __expf(lps);
                    a = lps - jsd_log_q(lps, lpt, ps, pt);
                }
                sg(c, ps > 0.f ? gscale * ps * (a - dot) : 0.f);
            }
        }
    } else {
        float tsum = 0.f;
#pragma unroll UR
        for (int c = 0; c < C; ++c) {
            const float t = lt(c);
            val += (t > 0.f ? t * __logf(t) : 0.f) - t * (ls(c) - lzs);
            tsum += t;
        }
        if (want_grad) {
#pragma unroll UR
            for (int c = 0; c < C; ++c) sg(c, gscale * (__expf(ls(c) - lzs) * tsum - lt(c)));
        }
    }
    return val;
}

struct PairNoPut { __device__ void operator()(int, float, float) const {} };
struct PairNoGet { __device__ void operator()(int, float &, float &) const {} };
constexpr PairNoPut pair_noput{};
constexpr PairNoGet pair_noget{};

template <int KIND>
__global__ __launch_bounds__(256) void pair_kernel(V3 s, V3 t, M3 g, float invT, float gscale, int N, int C, long long P, double *partial)
{
    double acc = 0.0;
    const long long total = (long long)N * P;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / P, p = i - n * P;
        const long long bs = n * s.sN + p * s.sP, bt = n * t.sN + p * t.sP, bg = n * g.sN + p * g.sP;
        const float tmul = KIND == PAIR_EKL ? 1.f : invT;
        acc += (double)pair_pixel<KIND, 0, false, 1>(
            C, [&](int c) { return kd_ld(s.p, s.dt, bs + c * s.sC) * invT; },
            [&](int c) { return kd_ld(t.p, t.dt, bt + c * t.sC) * tmul; },
            [&](int c, float v) { kd_st(g.p, g.dt, bg + c * g.sC, v); }, pair_noput, pair_noget, g.p != nullptr, gscale);
    }
    block_partials<1>({acc}, {partial});
}

// NHWC-dense fast path (the engine's logits layout): a block stages 256 pixels x C channels of both operands in LDS with fully
// coalesced loads, each thread then owns one pixel (row stride C words: conflict-free for odd C), and the gradient goes back out
// through the student's LDS rows, coalesced.
template <int KIND, typename TS, typename TT, typename TG>
__global__ __launch_bounds__(256) void pair_nhwc_kernel(const TS *__restrict__ s, const TT *__restrict__ t, TG *__restrict__ g, int C,
                                                        long long npix, float invT, float gscale, double *partial)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *ss = sm, *st = sm + 256 * C;
    double acc = 0.0;
    for (long long base = (long long)blockIdx.x * 256; base < npix; base += (long long)gridDim.x * 256) {
        const int np = (int)min((long long)256, npix - base);
        const int nel = np * C;
        stage_scaled(ss, s + base * C, nel, invT);
        stage_scaled(st, t + base * C, nel, KIND == PAIR_EKL ? 1.f : invT);
        __syncthreads();
        if ((int)threadIdx.x < np) {
            float *a = ss + threadIdx.x * C, *b = st + threadIdx.x * C;
            acc += (double)pair_pixel<KIND, 0, true, KIND == PAIR_KLD ? 8 : 1>(
                C, [&](int c) { return a[c]; }, [&](int c) { return b[c]; }, [&](int c, float v) { a[c] = v; },
                [&](int c, float ps, float av) { a[c] = ps; b[c] = av; }, [&](int c, float &ps, float &av) { ps = a[c]; av = b[c]; },
                g != nullptr, gscale);
        }
        __syncthreads();
        if (g) unstage(g + base * C, ss, nel);
        __syncthreads();
    }
    block_partials<1>({acc}, {partial});
}

// KLDiv / JSD from the two low-resolution logit tensors: ce2d_up_kernel's staging and interpolation, pair_pixel's arithmetic
template <int KIND, int CT>
__global__ __launch_bounds__(256) void pair_up_kernel(const float *__restrict__ s, const float *__restrict__ t, UpGeom g, float invT,
                                                      long long nchunks, int cpr, double *partial)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *ss = sm, *st = sm + 2 * UP_NW * g.C;
    double acc = 0.0;
    auto nostore = [](int, float) {};
    for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const UpChunk k = up_chunk(g, chunk, cpr);
        up_stage(ss, s, g, k.n, k.h0, k.h1, k.wlo, k.nw);
        up_stage(st, t, g, k.n, k.h0, k.h1, k.wlo, k.nw);
        __syncthreads();
        const int wo = k.wo0 + threadIdx.x;
        if (wo < g.W) {
            const UpCol col = up_col(g, k, wo);
            acc += (double)pair_pixel<KIND, CT, false, KIND == PAIR_KLD ? 4 : 1>(g.C, UpPix<CT>(ss, col, k.ah, invT), UpPix<CT>(st, col, k.ah, invT), nostore,
                                                       pair_noput, pair_noget, false, 0.f);
        }
        __syncthreads();
    }
    block_partials<1>({acc}, {partial});
}

// ---- focal loss (losses/FocalLoss.py:15-28) ------------------------------------------------------------------------------------
// Per pixel, with y' = y if y is a valid label else 0 (the gather index of FocalLoss.py:21):
//   a  = (1 - p_y')^gamma            (every pixel, ignored ones included)
//   ce = alpha_y * -log p_y           (valid pixels; 0 at ignored ones) and w = alpha_y (valid pixels)
// The three sums go to fixed-order partials; the finishing block writes stats = (sum a, sum ce, sum w) and the loss.
constexpr int FOCAL_MAX_BLOCKS = LOSS_FOCAL_MAX_BLOCKS;    // (one value, as MET_MAX_BLOCKS) three partial arrays inside kd_loss_workspace's 2 * LOSS_MAX_BLOCKS doubles

// x^g for x in [0, 1], g >= -1 through the hardware exp / log (powf is a long library sequence); 0^0 = 1 like torch.pow
__device__ __forceinline__ float focal_pow(float x, float g)
{
    if (g == 0.f) return 1.f;
    if (x <= 0.f) return g > 0.f ? 0.f : INFINITY;
    return __expf(g * __logf(x));
}

template <int CT, typename LX>
__device__ __forceinline__ void focal_pixel(int C_, LX lx, int y, bool valid, float wy, float gamma, float &a, float &ce)
{
    const int C = CT > 0 ? CT : C_;
    constexpr int UR = CT > 0 ? CT : 1;
    const int yg = valid ? y : 0;
    float m = -INFINITY;
#pragma unroll UR
    for (int c = 0; c < C; ++c) m = fmaxf(m, lx(c));
    float z = 0.f, vy = 0.f, eg = 0.f;
#pragma unroll UR
    for (int c = 0; c < C; ++c) {
        const float v = lx(c), e = __expf(v - m);
        z += e;
        eg = c == yg ? e : eg;
        vy = c == y ? v : vy;
    }
    a = focal_pow(1.f - eg / z, gamma);
    ce = valid ? wy * -(vy - m - __logf(z)) : 0.f;
}

__device__ __forceinline__ bool focal_valid(int64_t y, int ignore_index, int C) { return !(y == ignore_index || y < 0 || y >= C); }

__global__ __launch_bounds__(256) void focal_kernel(V3 x, const int64_t *__restrict__ target, const float *__restrict__ cw, float gamma,
                                                    int ignore_index, int N, int C, long long P, float *amap, float *cemap, double *partial)
{
    double sa = 0.0, sc = 0.0, sw = 0.0;
    const long long total = (long long)N * P;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int64_t y = target[i];
        const bool valid = focal_valid(y, ignore_index, C);
        const float wy = valid ? (cw ? cw[y] : 1.f) : 0.f;
        const long long n = i / P, p = i - n * P;
        const long long b = n * x.sN + p * x.sP;
        float a, ce;
        focal_pixel<0>(C, [&](int c) { return kd_ld(x.p, x.dt, b + c * x.sC); }, valid ? (int)y : 0, valid, wy, gamma, a, ce);
        if (amap) { amap[i] = a; cemap[i] = ce; }
        sa += (double)a; sc += (double)ce; sw += (double)wy;
    }
    block_partials<3>({sa, sc, sw}, {partial, partial + FOCAL_MAX_BLOCKS, partial + 2 * FOCAL_MAX_BLOCKS});
}

template <int CT>
__global__ __launch_bounds__(256) void focal_up_kernel(const float *__restrict__ x, const int64_t *__restrict__ target, const float *__restrict__ cw,
                                                       float gamma, int ignore_index, UpGeom g, long long nchunks, int cpr, double *partial)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    double sa = 0.0, sc = 0.0, sw = 0.0;
    for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const UpChunk k = up_chunk(g, chunk, cpr);
        up_stage(sm, x, g, k.n, k.h0, k.h1, k.wlo, k.nw);
        __syncthreads();
        const int wo = k.wo0 + threadIdx.x;
        if (wo < g.W) {
            const int64_t y = target[((size_t)k.n * g.H + k.ho) * g.W + wo];
            const bool valid = focal_valid(y, ignore_index, g.C);
            const float wy = valid ? (cw ? cw[y] : 1.f) : 0.f;
            float a, ce;
            focal_pixel<CT>(g.C, UpPix<CT>(sm, up_col(g, k, wo), k.ah), valid ? (int)y : 0, valid, wy, gamma, a, ce);
            sa += (double)a; sc += (double)ce; sw += (double)wy;
        }
        __syncthreads();
    }
    block_partials<3>({sa, sc, sw}, {partial, partial + FOCAL_MAX_BLOCKS, partial + 2 * FOCAL_MAX_BLOCKS});
}

// stats = (sum a, sum ce, sum w) in fixed order; loss: 'mean' mean(a) * (sum ce / sum w), 'sum' sum a * sum ce ('none': none)
__global__ __launch_bounds__(256) void focal_finish_kernel(const double *partial, int n, int reduction, double npix, double *stats, float *loss)
{
    __shared__ double sh[3][256];
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += 256)
        for (int q = 0; q < 3; ++q) v[q] += partial[q * FOCAL_MAX_BLOCKS + i];
    for (int q = 0; q < 3; ++q) sh[q][threadIdx.x] = v[q];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o)
            for (int q = 0; q < 3; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (stats) { stats[0] = sh[0][0]; stats[1] = sh[1][0]; stats[2] = sh[2][0]; }
        if (loss) *loss = (float)(reduction == 1 ? sh[0][0] / npix * (sh[1][0] / sh[2][0]) : sh[0][0] * sh[1][0]);
    }
}

// d loss / d x = u_a * da/dx + u_c * dce/dx, per pixel:
//   da/dx_c  = -gamma (1 - p_y')^(gamma-1) p_y' (delta_cy' - p_c)   (0 when gamma == 0, and when gamma < 1 at p_y' == 1, the limit)
//   dce/dx_c = alpha_y (p_c - delta_cy) at valid pixels, 0 at ignored ones
// 'mean': u_a = g * CE_mean / (N P), u_c = g * mean(a) / sum w;  'sum': u_a = g * CE_sum, u_c = g * sum a  (g: the upstream scalar)
// 'none': the loss is the (N,N,P) outer product L[i,j,p] = a[i,p] ce[j,p], so u_a[n,p] = sum_j G[n,j,p] ce[j,p] and
//         u_c[n,p] = sum_i G[i,n,p] a[i,p] with G the upstream (N,N,P) gradient
__global__ __launch_bounds__(256) void focal_grad_kernel(V3 x, const int64_t *__restrict__ target, const float *__restrict__ cw, float gamma,
                                                         int ignore_index, int reduction, int N, int C, long long P, const double *stats,
                                                         const float *up, const float *amap, const float *cemap, M3 g)
{
    float ua = 0.f, uc = 0.f;
    if (reduction != 0) {
        const double gu = (double)up[0], sa = stats[0], sc = stats[1], sw = stats[2], np = (double)N * (double)P;
        ua = (float)(reduction == 1 ? gu * (sc / sw) / np : gu * sc);
        uc = (float)(reduction == 1 ? gu * (sa / np) / sw : gu * sa);
    }
    const long long total = (long long)N * P;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long n = i / P, p = i - n * P;
        if (reduction == 0) {
            float fa = 0.f, fc = 0.f;
            for (int j = 0; j < N; ++j) {
                fa += up[((long long)n * N + j) * P + p] * cemap[(long long)j * P + p];
                fc += up[((long long)j * N + n) * P + p] * amap[(long long)j * P + p];
            }
            ua = fa; uc = fc;
        }
        const int64_t y = target[i];
        const bool valid = focal_valid(y, ignore_index, C);
        const int yg = valid ? (int)y : 0;
        const float wy = valid ? (cw ? cw[y] : 1.f) : 0.f;
        const long long b = n * x.sN + p * x.sP, gb = n * g.sN + p * g.sP;
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) m = fmaxf(m, kd_ld(x.p, x.dt, b + c * x.sC));
        float z = 0.f;
        for (int c = 0; c < C; ++c) z += __expf(kd_ld(x.p, x.dt, b + c * x.sC) - m);
        const float iz = 1.f / z;
        const float pg = __expf(kd_ld(x.p, x.dt, b + yg * x.sC) - m) * iz, om = 1.f - pg;
        const float da = (gamma == 0.f || (om <= 0.f && gamma < 1.f)) ? 0.f : -gamma * focal_pow(om, gamma - 1.f) * pg;
        const float ka = ua * da, kc = uc * wy;
        for (int c = 0; c < C; ++c) {
            const float pc = __expf(kd_ld(x.p, x.dt, b + c * x.sC) - m) * iz;
            kd_st(g.p, g.dt, gb + c * g.sC, ka * ((c == yg ? 1.f : 0.f) - pc) + kc * (pc - (c == yg && valid ? 1.f : 0.f)));
        }
    }
}

// ---- top-k hint MSE (losses/WeightedHintMSELoss.py:19-44) ------------------------------------------------------------------------
// 1. topk_sums_kernel: per (n, c, pixel chunk) sums of t^2 and (s-t)^2 from one read of s and t.  grid (chunks, ceil(C/64), N);
//    thread = channel (tid & 63) x pixel lane (tid >> 6, every 4th pixel of the chunk); the 4 lanes are added in a fixed order.
// 2. topk_select_kernel: one 1024-thread block per sample; channel sums in fixed chunk order, then rank by count in LDS:
//    rank(c) = #{c' : v[c'] > v[c] or (v[c'] == v[c] and c' < c)}, kept iff rank < K (ties: the lower channel first).
//    Writes the (N,C) mask and the sample's sum over kept channels of sum_p (s-t)^2.
// 3. topk_grad_kernel: grad = gscale * mask * (s - t).

__global__ __launch_bounds__(256) void topk_sums_kernel(V3 s, V3 t, int C, long long P, long long per_chunk, int nchunk, double *pt2, double *pd2)
{
    __shared__ double sh[2][4][64];
    const int ci = threadIdx.x & 63, pj = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + ci, n = blockIdx.z, chunk = blockIdx.x;
    double dt2 = 0.0, dd2 = 0.0;
    if (c < C) {
        const long long p0 = (long long)chunk * per_chunk, p1 = min(P, p0 + per_chunk);
        const long long bs = n * s.sN + c * s.sC, bt = n * t.sN + c * t.sC;
        // fp64 accumulation: the ranking compares these sums, and neighbouring norms of a wide hint can be 1e-6 apart
        for (long long p = p0 + pj; p < p1; p += 4) {
            const float tv = kd_ld(t.p, t.dt, bt + p * t.sP), d = kd_ld(s.p, s.dt, bs + p * s.sP) - tv;
            dt2 = fma((double)tv, (double)tv, dt2);
            dd2 = fma((double)d, (double)d, dd2);
        }
    }
    sh[0][pj][ci] = dt2; sh[1][pj][ci] = dd2;
    __syncthreads();
    if (pj == 0 && c < C) {
        const long long o = ((long long)n * C + c) * nchunk + chunk;
        pt2[o] = ((sh[0][0][ci] + sh[0][1][ci]) + sh[0][2][ci]) + sh[0][3][ci];
        pd2[o] = ((sh[1][0][ci] + sh[1][1][ci]) + sh[1][2][ci]) + sh[1][3][ci];
    }
}

__global__ __launch_bounds__(1024) void topk_select_kernel(const double *pt2, const double *pd2, int C, int nchunk, int K, float *mask,
                                                           double *partial)
{
    extern __shared__ double v[];
    __shared__ double wsum[16];
    const int n = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 1024) {
        const double *q = pt2 + ((long long)n * C + c) * nchunk;
        double a = 0.0;
        for (int k = 0; k < nchunk; ++k) a += q[k];
        v[c] = a;
    }
    __syncthreads();
    double contrib = 0.0;
    for (int c = threadIdx.x; c < C; c += 1024) {
        const double vc = v[c];
        int rank = 0;
        for (int j = 0; j < C; ++j) {
            const double vj = v[j];
            rank += (vj > vc || (vj == vc && j < c)) ? 1 : 0;
        }
        const bool keep = rank < K;
        mask[(long long)n * C + c] = keep ? 1.f : 0.f;
        if (keep) {
            const double *q = pd2 + ((long long)n * C + c) * nchunk;
            double d = 0.0;
            for (int k = 0; k < nchunk; ++k) d += q[k];
            contrib += d;
        }
    }
    contrib = wave_sum_d(contrib);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = contrib;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < 16; ++w) s += wsum[w];
        partial[n] = s;
    }
}

// dense fast path (s, t, g share one dense layout, as dense_same checks): 8 elements per thread and step, all in one (n, c) row
// of the mask -- CFAST (NHWC): C % 8 == 0, the 8 are consecutive channels of one pixel; else (NCHW): P % 8 == 0, one channel
template <typename T, bool CFAST>
__global__ __launch_bounds__(256) void topk_grad_vec_kernel(const T *__restrict__ s, const T *__restrict__ t, T *__restrict__ g,
                                                            const float *__restrict__ mask, float gscale, int C, long long P, long long n8)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        const long long e = i * 8;
        float mk[8];
        if constexpr (CFAST) {
            const long long pix = e / C, c0 = e - pix * C, n = pix / P;
            const float4 m0 = *(const float4 *)(mask + n * C + c0), m1 = *(const float4 *)(mask + n * C + c0 + 4);
            mk[0] = m0.x; mk[1] = m0.y; mk[2] = m0.z; mk[3] = m0.w; mk[4] = m1.x; mk[5] = m1.y; mk[6] = m1.z; mk[7] = m1.w;
        } else {
            const float m = mask[e / P];
#pragma unroll
            for (int q = 0; q < 8; ++q) mk[q] = m;
        }
        float a[8], b[8], d[8];
        ld8(s + e, a);
        ld8(t + e, b);
#pragma unroll
        for (int q = 0; q < 8; ++q) d[q] = mk[q] != 0.f ? gscale * mk[q] * (a[q] - b[q]) : 0.f;
        st8(g + e, d);
    }
}

__global__ __launch_bounds__(256) void topk_grad_kernel(V3 s, V3 t, M3 g, const float *mask, float gscale, int N, int C, long long P, int c_fast)
{
    const long long total = (long long)N * C * P;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long n, c, p;
        if (c_fast) { c = i % C; const long long r = i / C; p = r % P; n = r / P; }
        else { p = i % P; const long long r = i / P; c = r % C; n = r / C; }
        const float mk = mask[n * C + c];
        const float d = mk != 0.f ? kd_ld(s.p, s.dt, n * s.sN + c * s.sC + p * s.sP) - kd_ld(t.p, t.dt, n * t.sN + c * t.sC + p * t.sP) : 0.f;
        kd_st(g.p, g.dt, n * g.sN + c * g.sC + p * g.sP, gscale * mk * d);
    }
}

// ---- multi-target KL + cross entropy in one pass (kd_kldiv_multi) and the ensemble's mean softmax (kd_softmax_mean) ----------------
// trainer/ensemble_trainer.py:80-85 back-propagates sum_k w_k KLDiv(s, t_k) / W + CE(s, y); its gradient is linear in the targets:
//   gk * (softmax(s/T) - sum_k w_k softmax(t_k/T) / W) + gs * (softmax(s) - onehot)
// so the student row is read once, every target row once (its KL value accumulated per target, its probabilities into q) and the
// gradient is written once.  The target views travel by value in the kernel argument (w already divided by W).  Three shapes:
//   mt_wave_kernel   class stride 1, a row of C <= 1024 classes held in one wave's registers, reductions by lane shuffles;
//   kldm_nhwc_kernel dense NHWC with few classes and many pixels: 256 pixels per block staged through LDS, one pixel per thread;
//   kldm_kernel      any strides / any C: one pixel per thread, the operands re-read from cache as pair_kernel does.
struct MT { V3 t[KD_MULTI_MAX]; float w[KD_MULTI_MAX]; int n; };

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// sup_scale / #valid from the count partials: every wave adds them in the same order, so every wave holds the same bits
__device__ __forceinline__ float mt_sup_scale(const double *count, int ncount, float sup_scale)
{
    double c = 0.0;
    for (int i = threadIdx.x & 63; i < ncount; i += 64) c += count[i];
    c = wave_sum_d(c);
    return c > 0.0 ? sup_scale / (float)c : 0.f;
}

// A row of C classes in one wave: lane l holds 4 * NCH elements.  VEC: element (j, q) is class (j * 64 + l) * 4 + q, one 16-B (fp32)
// or 8-B (bf16) access per j (C % 4 == 0, the row 4-element aligned); otherwise class (j * 4 + q) * 64 + l, scalar and coalesced.
template <bool VEC> __device__ __forceinline__ int row_cls(int j, int q, int lane)
{
    return VEC ? (j * 64 + lane) * 4 + q : (j * 4 + q) * 64 + lane;
}
template <int NCH, bool VEC>
__device__ __forceinline__ void row_load(const void *p, int dt, long long base, int C, int lane, float (&v)[NCH * 4])
{
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        if (VEC) {
            const int c0 = (j * 64 + lane) * 4;
            if (c0 < C) {
                if (dt == KD_BF16) {
                    const uint2 u = *(const uint2 *)((const bf16_t *)p + base + c0);
                    v[j * 4] = __uint_as_float(u.x << 16); v[j * 4 + 1] = __uint_as_float(u.x & 0xffff0000u);
                    v[j * 4 + 2] = __uint_as_float(u.y << 16); v[j * 4 + 3] = __uint_as_float(u.y & 0xffff0000u);
                } else {
                    const float4 f = *(const float4 *)((const float *)p + base + c0);
                    v[j * 4] = f.x; v[j * 4 + 1] = f.y; v[j * 4 + 2] = f.z; v[j * 4 + 3] = f.w;
                }
            } else {
                v[j * 4] = v[j * 4 + 1] = v[j * 4 + 2] = v[j * 4 + 3] = -INFINITY;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = (j * 4 + q) * 64 + lane;
                v[j * 4 + q] = c < C ? kd_ld(p, dt, base + c) : -INFINITY;
            }
        }
    }
}
template <int NCH, bool VEC>
__device__ __forceinline__ void row_store(void *p, int dt, long long base, int C, int lane, const float (&v)[NCH * 4])
{
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        if (VEC) {
            const int c0 = (j * 64 + lane) * 4;
            if (c0 < C) {
                if (dt == KD_BF16)
                    *(uint2 *)((bf16_t *)p + base + c0) = make_uint2(pack_bf16x2(v[j * 4], v[j * 4 + 1]), pack_bf16x2(v[j * 4 + 2], v[j * 4 + 3]));
                else
                    *(float4 *)((float *)p + base + c0) = make_float4(v[j * 4], v[j * 4 + 1], v[j * 4 + 2], v[j * 4 + 3]);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = (j * 4 + q) * 64 + lane;
                if (c < C) kd_st(p, dt, base + c, v[j * 4 + q]);
            }
        }
    }
}

// one target row: q += w * softmax(t / T); returns this lane's share of sum_c pt (lpt - lps) when lps is given
template <int NCH, bool VEC, bool WITH_KL>
__device__ __forceinline__ float row_target(const V3 &t, long long n, long long p, int C, int lane, float invT, float w,
                                            const float (&lps)[NCH * 4], float (&q)[NCH * 4])
{
    constexpr int E = NCH * 4;
    float xt[E];
    row_load<NCH, VEC>(t.p, t.dt, n * t.sN + p * t.sP, C, lane, xt);
    float m = -INFINITY;
#pragma unroll
    for (int e = 0; e < E; ++e) m = fmaxf(m, xt[e]);
    const float mt = wave_max(m) * invT;
    float z = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) z += __expf(xt[e] * invT - mt);
    const float lzt = __logf(wave_sum(z)) + mt;
    float kl = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const float lpt = xt[e] * invT - lzt, pt = __expf(lpt);
        if (WITH_KL) kl += pt > 0.f ? pt * (lpt - lps[e]) : 0.f;
        q[e] += w * pt;
    }
    return kl;
}

// SMEAN: kd_softmax_mean (s unused, g = the fp32 output); otherwise kd_kldiv_multi
template <int NCH, bool VEC, bool SMEAN>
__global__ __launch_bounds__(256) void mt_wave_kernel(V3 s, const MT tg, M3 g, const int64_t *__restrict__ labels, int ignore_index,
                                                      float invT, float gk, float sup_scale, int C, long long P, long long rows,
                                                      const double *count, int ncount, double *pkd, double *pce)
{
    constexpr int E = NCH * 4;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float gs = (!SMEAN && labels) ? mt_sup_scale(count, ncount, sup_scale) : 0.f;
    double akd = 0.0, ace = 0.0;
    for (long long row = (long long)blockIdx.x * 4 + wv; row < rows; row += (long long)gridDim.x * 4) {
        const long long n = row / P, p = row - n * P;
        float sr[E], lps[E], q[E];
#pragma unroll
        for (int e = 0; e < E; ++e) { q[e] = 0.f; lps[e] = 0.f; sr[e] = 0.f; }
        float lz1 = 0.f;
        bool valid = false;
        int y = -1;
        if (!SMEAN) {
            row_load<NCH, VEC>(s.p, s.dt, n * s.sN + p * s.sP, C, lane, sr);
            float m = -INFINITY;
#pragma unroll
            for (int e = 0; e < E; ++e) m = fmaxf(m, sr[e]);
            m = wave_max(m);
            const float ms = m * invT;
            float z = 0.f;
#pragma unroll
            for (int e = 0; e < E; ++e) z += __expf(sr[e] * invT - ms);
            const float lzs = __logf(wave_sum(z)) + ms;
#pragma unroll
            for (int e = 0; e < E; ++e) lps[e] = sr[e] * invT - lzs;
            lz1 = lzs;
            if (labels) {
                const int64_t yy = labels[row];
                valid = !(yy == ignore_index || yy < 0 || yy >= C);      // (one row per wave: uniform)
                y = (int)yy;
                if (valid) {
                    if (invT != 1.f) {
                        float z1 = 0.f;
#pragma unroll
                        for (int e = 0; e < E; ++e) z1 += __expf(sr[e] - m);
                        lz1 = __logf(wave_sum(z1)) + m;
                    }
#pragma unroll
                    for (int e = 0; e < E; ++e)
                        if (row_cls<VEC>(e >> 2, e & 3, lane) == y) ace += (double)(lz1 - sr[e]);
                }
            }
        }
        float kl = 0.f;
        for (int k = 0; k < tg.n; ++k) kl += tg.w[k] * row_target<NCH, VEC, !SMEAN>(tg.t[k], n, p, C, lane, invT, tg.w[k], lps, q);
        akd += (double)kl;
        if (g.p) {
            if (!SMEAN) {
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    float v = gk * (__expf(lps[e]) - q[e]);
                    if (valid) v += gs * (__expf(sr[e] - lz1) - (row_cls<VEC>(e >> 2, e & 3, lane) == y ? 1.f : 0.f));
                    q[e] = v;
                }
            }
            row_store<NCH, VEC>(g.p, g.dt, n * g.sN + p * g.sP, C, lane, q);
        }
    }
    if (!SMEAN) block_partials<2>({akd, ace}, {pkd, pce});
}

// global <-> LDS staging of `nel` consecutive elements of either storage type: 16-B accesses when the chunk is whole and aligned
__device__ __forceinline__ void stage_any(float *dst, const void *src, int dt, long long off, int nel)
{
    if (dt == KD_BF16) {
        const bf16_t *sp = (const bf16_t *)src + off;
        if ((nel & 7) == 0 && ((uintptr_t)sp & 15) == 0) {
            for (int i = threadIdx.x; i < (nel >> 3); i += 256) {
                float v[8];
                ld8(sp + i * 8, v);
                ((float4 *)dst)[i * 2] = make_float4(v[0], v[1], v[2], v[3]);
                ((float4 *)dst)[i * 2 + 1] = make_float4(v[4], v[5], v[6], v[7]);
            }
        } else {
            for (int i = threadIdx.x; i < nel; i += 256) dst[i] = bf16_to_f32(sp[i]);
        }
    } else {
        stage_scaled(dst, (const float *)src + off, nel, 1.0f);
    }
}
__device__ __forceinline__ void unstage_any(void *dst, int dt, long long off, const float *src, int nel)
{
    if (dt == KD_BF16) {
        bf16_t *dp = (bf16_t *)dst + off;
        if ((nel & 7) == 0 && ((uintptr_t)dp & 15) == 0) {
            for (int i = threadIdx.x; i < (nel >> 3); i += 256) {
                const float4 a = ((const float4 *)src)[i * 2], b = ((const float4 *)src)[i * 2 + 1];
                const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
                st8(dp + i * 8, v);
            }
        } else {
            for (int i = threadIdx.x; i < nel; i += 256) dp[i] = f32_to_bf16(src[i]);
        }
    } else {
        unstage((float *)dst + off, src, nel);
    }
}

// dense NHWC, 3 * 256 * C floats of LDS (student rows, the current target's rows, q / the gradient)
__global__ __launch_bounds__(256) void kldm_nhwc_kernel(V3 s, const MT tg, M3 g, const int64_t *__restrict__ labels, int ignore_index,
                                                        float invT, float gk, float sup_scale, int C, long long npix,
                                                        const double *count, int ncount, double *pkd, double *pce)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *A = sm, *B = sm + 256 * C, *Q = sm + 512 * C;
    const float gs = labels ? mt_sup_scale(count, ncount, sup_scale) : 0.f;
    double akd = 0.0, ace = 0.0;
    for (long long base = (long long)blockIdx.x * 256; base < npix; base += (long long)gridDim.x * 256) {
        const int np = (int)min((long long)256, npix - base);
        const int nel = np * C;
        const bool mine = (int)threadIdx.x < np;
        float *a = A + threadIdx.x * C, *b = B + threadIdx.x * C, *q = Q + threadIdx.x * C;
        float lzs = 0.f, lz1 = 0.f, kl = 0.f;
        bool valid = false;
        int y = -1;
        stage_any(A, s.p, s.dt, base * C, nel);
        for (int k = 0; k < tg.n; ++k) {
            stage_any(B, tg.t[k].p, tg.t[k].dt, base * C, nel);
            __syncthreads();
            if (mine && k == 0) {
                float m = -INFINITY;
                for (int c = 0; c < C; ++c) m = fmaxf(m, a[c]);
                const float ms = m * invT;
                float z = 0.f;
                for (int c = 0; c < C; ++c) { z += __expf(a[c] * invT - ms); q[c] = 0.f; }
                lzs = __logf(z) + ms;
                lz1 = lzs;
                if (labels) {
                    const int64_t yy = labels[base + threadIdx.x];
                    valid = !(yy == ignore_index || yy < 0 || yy >= C);
                    y = (int)yy;
                    if (valid) {
                        if (invT != 1.f) {
                            float z1 = 0.f;
                            for (int c = 0; c < C; ++c) z1 += __expf(a[c] - m);
                            lz1 = __logf(z1) + m;
                        }
                        ace += (double)(lz1 - a[y]);
                    }
                }
            }
            if (mine) {
                const float w = tg.w[k];
                float m = -INFINITY;
                for (int c = 0; c < C; ++c) m = fmaxf(m, b[c]);
                const float mt = m * invT;
                float z = 0.f;
                for (int c = 0; c < C; ++c) z += __expf(b[c] * invT - mt);
                const float lzt = __logf(z) + mt;
                float klk = 0.f;
                for (int c = 0; c < C; ++c) {
                    const float lpt = b[c] * invT - lzt, pt = __expf(lpt);
                    klk += pt > 0.f ? pt * (lpt - (a[c] * invT - lzs)) : 0.f;
                    q[c] += w * pt;
                }
                kl += w * klk;
            }
            __syncthreads();
        }
        akd += (double)kl;
        if (g.p) {
            if (mine) {
                for (int c = 0; c < C; ++c) {
                    float v = gk * (__expf(a[c] * invT - lzs) - q[c]);
                    if (valid) v += gs * (__expf(a[c] - lz1) - (c == y ? 1.f : 0.f));
                    q[c] = v;
                }
            }
            __syncthreads();
            unstage_any(g.p, g.dt, base * C, Q, nel);
        }
        __syncthreads();
    }
    block_partials<2>({akd, ace}, {pkd, pce});
}

// any strides, any C: one pixel per thread; log Z of every target parked in LDS ([target][thread]: conflict-free)
template <bool SMEAN>
__global__ __launch_bounds__(256) void kldm_kernel(V3 s, const MT tg, M3 g, const int64_t *__restrict__ labels, int ignore_index, float invT,
                                                   float gk, float sup_scale, int C, long long P, long long rows, const double *count,
                                                   int ncount, double *pkd, double *pce)
{
    __shared__ float lz[KD_MULTI_MAX][256];
    const float gs = (!SMEAN && labels) ? mt_sup_scale(count, ncount, sup_scale) : 0.f;
    double akd = 0.0, ace = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < rows; i += (long long)gridDim.x * 256) {
        const long long n = i / P, p = i - n * P;
        const long long bs = n * s.sN + p * s.sP, bg = n * g.sN + p * g.sP;
        float lzs = 0.f, lz1 = 0.f;
        bool valid = false;
        int y = -1;
        if (!SMEAN) {
            float m = -INFINITY;
            for (int c = 0; c < C; ++c) m = fmaxf(m, kd_ld(s.p, s.dt, bs + c * s.sC));
            const float ms = m * invT;
            float z = 0.f;
            for (int c = 0; c < C; ++c) z += __expf(kd_ld(s.p, s.dt, bs + c * s.sC) * invT - ms);
            lzs = __logf(z) + ms;
            lz1 = lzs;
            if (labels) {
                const int64_t yy = labels[i];
                valid = !(yy == ignore_index || yy < 0 || yy >= C);
                y = (int)yy;
                if (valid) {
                    if (invT != 1.f) {
                        float z1 = 0.f;
                        for (int c = 0; c < C; ++c) z1 += __expf(kd_ld(s.p, s.dt, bs + c * s.sC) - m);
                        lz1 = __logf(z1) + m;
                    }
                    ace += (double)(lz1 - kd_ld(s.p, s.dt, bs + y * s.sC));
                }
            }
        }
        for (int k = 0; k < tg.n; ++k) {
            const V3 t = tg.t[k];
            const long long bt = n * t.sN + p * t.sP;
            float m = -INFINITY;
            for (int c = 0; c < C; ++c) m = fmaxf(m, kd_ld(t.p, t.dt, bt + c * t.sC));
            const float mt = m * invT;
            float z = 0.f;
            for (int c = 0; c < C; ++c) z += __expf(kd_ld(t.p, t.dt, bt + c * t.sC) * invT - mt);
            lz[k][threadIdx.x] = __logf(z) + mt;
        }
        float kl = 0.f;
        for (int c = 0; c < C; ++c) {
            const float sv = SMEAN ? 0.f : kd_ld(s.p, s.dt, bs + c * s.sC);
            const float lps = sv * invT - lzs;
            float q = 0.f;
            for (int k = 0; k < tg.n; ++k) {
                const V3 t = tg.t[k];
                const float lpt = kd_ld(t.p, t.dt, n * t.sN + p * t.sP + c * t.sC) * invT - lz[k][threadIdx.x], pt = __expf(lpt);
                if (!SMEAN) kl += tg.w[k] * (pt > 0.f ? pt * (lpt - lps) : 0.f);
                q += tg.w[k] * pt;
            }
            if (g.p) {
                float v = q;
                if (!SMEAN) {
                    v = gk * (__expf(lps) - q);
                    if (valid) v += gs * (__expf(sv - lz1) - (c == y ? 1.f : 0.f));
                }
                kd_st(g.p, g.dt, bg + c * g.sC, v);
            }
        }
        akd += (double)kl;
    }
    if (!SMEAN) block_partials<2>({akd, ace}, {pkd, pce});
}

// out[0] = kd, out[1] = sup, out[2] = kd_scale * kd + sup_scale * sup
__global__ __launch_bounds__(256) void mt_finish_kernel(const double *pkd, const double *pce, int n, const double *count, int ncount,
                                                        double kd_mul, float kd_scale, float sup_scale, float *out)
{
    __shared__ double sh[3][256];
    double a = 0.0, b = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) { a += pkd[i]; b += pce[i]; }
    for (int i = threadIdx.x; i < ncount; i += 256) c += count[i];
    sh[0][threadIdx.x] = a; sh[1][threadIdx.x] = b; sh[2][threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o)
            for (int r = 0; r < 3; ++r) sh[r][threadIdx.x] += sh[r][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float kd = (float)(sh[0][0] * kd_mul);
        const float sup = sh[2][0] > 0.0 ? (float)(sh[1][0] / sh[2][0]) : 0.f;
        out[0] = kd; out[1] = sup; out[2] = kd_scale * kd + sup_scale * sup;
    }
}

}  // namespace

// ---- the launchers ---------------------------------------------------------------------------------------------------------------
// Each entry point checks its arguments, asks the selector of its family (loss_select.h) for the kernel, the grid and the dynamic
// LDS, notes the kernel's name once and switches over it.
static_assert((int)PAIR_KLD == LOSS_KLD && (int)PAIR_JSD == LOSS_JSD && (int)PAIR_EKL == LOSS_EKL,
              "loss_select.h numbers the two-operand criteria like the kernels' template argument");

namespace {
// A missing kernel is an error, never a silent no-op: a value the family's selector should not return, or one this file was not
// taught to launch, ends the call here.
int no_launch(const char *who, const LossSel &sel)
{
    kd_set_error("%s: no launch for kernel %d", who, (int)sel.kernel);
    return KD_ERR_UNSUPPORTED;
}
// the function to launch for `k`, from (value, function of one signature) pairs; null if k is none of them
template <typename F> F launch_of(LossKernel) { return nullptr; }
template <typename F, typename... R> F launch_of(LossKernel k, LossKernel ka, F a, R... rest) { return k == ka ? a : launch_of<F>(k, rest...); }
}  // namespace

extern "C" size_t kd_loss_workspace(int32_t N, int32_t C, int64_t P) { return loss_workspace_bytes(N, C, P); }

#define KD_LOSS_COMMON(who)                                                                                          \
    KD_REQUIRE(s && t && s->ptr && t->ptr && loss && workspace, KD_ERR_INVALID, who ": null argument");              \
    KD_REQUIRE(ok_dt(s->dtype) && ok_dt(t->dtype) && (!grad || ok_dt(grad->dtype)), KD_ERR_INVALID, who ": bad dtype"); \
    KD_REQUIRE(N > 0 && C > 0 && P > 0, KD_ERR_INVALID, who ": bad shape");                                          \
    KD_REQUIRE(workspace_bytes >= kd_loss_workspace(N, C, P), KD_ERR_WORKSPACE, who ": workspace too small");        \
    KD_REQUIRE(((uintptr_t)workspace & 7) == 0, KD_ERR_INVALID, who ": workspace must be 8-B aligned")

// ---- kd_kldiv / kd_jsdiv / kd_ensemble_kldiv: the entry point sets the scales ----------------------------------------------------
namespace {
using PairNhwcLaunch = void (*)(const LossSel &, hipStream_t, const void *, const void *, void *, int, long long, float, float, double *);
template <int K, typename TS, typename TT, typename TG>
void pair_nhwc_launch(const LossSel &sel, hipStream_t st, const void *s, const void *t, void *g, int C, long long npix, float invT, float gscale,
                      double *partial)
{
    hipLaunchKernelGGL((pair_nhwc_kernel<K, TS, TT, TG>), dim3(sel.blocks), dim3(256), sel.lds, st, (const TS *)s, (const TT *)t, (TG *)g, C, npix,
                       invT, gscale, partial);
}
// in the order of LK_PAIR_NHWC .. LK_PAIR_NHWC_LAST: the kind, then the storage of s, t and the gradient, fp32 before bf16
#define KD_PAIR_FORMS(K)                                                                                                           \
    pair_nhwc_launch<K, float, float, float>, pair_nhwc_launch<K, float, float, bf16_t>, pair_nhwc_launch<K, float, bf16_t, float>, \
    pair_nhwc_launch<K, float, bf16_t, bf16_t>, pair_nhwc_launch<K, bf16_t, float, float>, pair_nhwc_launch<K, bf16_t, float, bf16_t>, \
    pair_nhwc_launch<K, bf16_t, bf16_t, float>, pair_nhwc_launch<K, bf16_t, bf16_t, bf16_t>
const PairNhwcLaunch pair_nhwc_launches[] = {KD_PAIR_FORMS(PAIR_KLD), KD_PAIR_FORMS(PAIR_JSD), KD_PAIR_FORMS(PAIR_EKL)};
#undef KD_PAIR_FORMS
static_assert(sizeof(pair_nhwc_launches) / sizeof(pair_nhwc_launches[0]) == LK_PAIR_NHWC_LAST - LK_PAIR_NHWC + 1, "a launch per channels-last form");
}  // namespace

static int pair_impl(const char *who, int kind, const kd_view3 *s, const kd_view3 *t, float invT, int32_t N, int32_t C, int64_t P,
                     float *loss, const kd_mview3 *grad, float gscale, double loss_scale, void *workspace, kd_stream_t stream)
{
    double *partial = (double *)workspace;
    hipStream_t st = (hipStream_t)stream;
    const LossSel sel = loss_select_pair((LossPair)kind, s, t, grad, N, C, P);
    KD_NOTE_PLUMBING(loss_kernel_name(sel.kernel));
    if (sel.kernel >= LK_PAIR_NHWC && sel.kernel <= LK_PAIR_NHWC_LAST) {
        pair_nhwc_launches[sel.kernel - LK_PAIR_NHWC](sel, st, s->ptr, t->ptr, grad ? grad->ptr : nullptr, C, (long long)N * P, invT, gscale, partial);
    } else {
        auto fn = launch_of(sel.kernel, LK_PAIR_KLD, pair_kernel<PAIR_KLD>, LK_PAIR_JSD, pair_kernel<PAIR_JSD>, LK_PAIR_EKL, pair_kernel<PAIR_EKL>);
        if (!fn) return no_launch(who, sel);
        hipLaunchKernelGGL(fn, dim3(sel.blocks), dim3(256), 0, st, v3(s), v3(t), m3(grad), invT, gscale, N, C, (long long)P, partial);
    }
    KD_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(256), 0, st, (const double *)partial, sel.blocks, loss_scale, (const double *)nullptr, loss);
    KD_CHECK_LAUNCH(who);
    return KD_OK;
}

extern "C" int kd_kldiv(const kd_view3 *s, const kd_view3 *t, float temperature, int32_t N, int32_t C, int64_t P, float *loss,
                        const kd_mview3 *grad, float grad_scale, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    KD_LOSS_COMMON("kd_kldiv");
    KD_REQUIRE(temperature > 0.f, KD_ERR_INVALID, "kd_kldiv: temperature must be positive");
    const float gscale = grad_scale * temperature / ((float)N * (float)P);
    // 'mean' over N*C*P elements, then * T^2 * C  ==  T^2 / (N*P) * sum
    const double scale = (double)temperature * temperature / ((double)N * (double)P);
    return pair_impl("kd_kldiv", PAIR_KLD, s, t, 1.f / temperature, N, C, P, loss, grad, gscale, scale, workspace, stream);
}

extern "C" int kd_jsdiv(const kd_view3 *s, const kd_view3 *t, float temperature, int32_t N, int32_t C, int64_t P, float *loss,
                        const kd_mview3 *grad, float grad_scale, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    KD_LOSS_COMMON("kd_jsdiv");
    KD_REQUIRE(temperature > 0.f, KD_ERR_INVALID, "kd_jsdiv: temperature must be positive");
    // loss = T^2 / (2N) * sum ; d/ds = T / (2N) * ps (a - <ps, a>)   (divided by the batch size only, losses/JSDiv.py:24-25)
    const float gscale = grad_scale * temperature / (2.f * (float)N);
    const double scale = (double)temperature * temperature / (2.0 * (double)N);
    return pair_impl("kd_jsdiv", PAIR_JSD, s, t, 1.f / temperature, N, C, P, loss, grad, gscale, scale, workspace, stream);
}

extern "C" int kd_ensemble_kldiv(const kd_view3 *s, const kd_view3 *t, int32_t N, int32_t C, int64_t P, float *loss, const kd_mview3 *grad,
                                 float grad_scale, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    KD_LOSS_COMMON("kd_ensemble_kldiv");
    // 'mean' over N*C*P elements, then * C  ==  1 / (N*P) * sum
    const float gscale = grad_scale / ((float)N * (float)P);
    const double scale = 1.0 / ((double)N * (double)P);
    return pair_impl("kd_ensemble_kldiv", PAIR_EKL, s, t, 1.f, N, C, P, loss, grad, gscale, scale, workspace, stream);
}

extern "C" int kd_hint_mse(const kd_view3 *s, const kd_view3 *t, float num_classes, int32_t N, int32_t C, int64_t P,
                           float *loss, const kd_mview3 *grad, float grad_scale, void *workspace, size_t workspace_bytes,
                           kd_stream_t stream)
{
    KD_LOSS_COMMON("kd_hint_mse");
    double *partial = (double *)workspace;
    const long long numel = (long long)N * C * P;
    const float gscale = grad_scale * 2.f * num_classes / (float)numel;
    hipStream_t st = (hipStream_t)stream;
    const LossSel sel = loss_select_mse(s, t, grad, N, C, P);
    KD_NOTE_PLUMBING(loss_kernel_name(sel.kernel));
    auto vec = [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(mse_vec_kernel<T>, dim3(sel.blocks), dim3(256), 0, st, (const T *)s->ptr, (const T *)t->ptr,
                           (T *)(grad ? grad->ptr : nullptr), gscale, numel / 8, partial);
    };
    switch (sel.kernel) {
    case LK_MSE_VEC_F32: vec(float{}); break;
    case LK_MSE_VEC_BF16: vec(bf16_t{}); break;
    case LK_MSE_STRIDED:
        hipLaunchKernelGGL(mse_strided_kernel, dim3(sel.blocks), dim3(256), 0, st, v3(s), v3(t), m3(grad), gscale, N, C, (long long)P,
                           s->sC == 1 ? 1 : 0, partial);
        break;
    default: return no_launch("kd_hint_mse", sel);
    }
    KD_CHECK_LAUNCH("kd_hint_mse");
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(256), 0, st, (const double *)partial, sel.blocks, (double)num_classes / (double)numel,
                       (const double *)nullptr, loss);
    KD_CHECK_LAUNCH("kd_hint_mse(finish)");
    return KD_OK;
}

extern "C" int kd_weighted_hint_mse(const kd_view3 *s, const kd_view3 *t, const float *w, int32_t w_per_sample, int32_t N,
                                    int32_t C, int64_t P, float *loss, const kd_mview3 *grad, float grad_scale, void *workspace,
                                    size_t workspace_bytes, kd_stream_t stream)
{
    KD_LOSS_COMMON("kd_weighted_hint_mse");
    KD_REQUIRE(w, KD_ERR_INVALID, "kd_weighted_hint_mse: null weight");
    hipStream_t st = (hipStream_t)stream;
    const LossSel sel = loss_select_whmse(N, C, P);
    const dim3 grid((unsigned)sel.chunks, (unsigned)((C + 255) / 256), (unsigned)N);
    double *partial = (double *)workspace;
    float *wsum = (float *)((char *)workspace + sel.aux_off);
    KD_NOTE_PLUMBING(loss_kernel_name(LK_WHMSE));      // the one kernel; the selector plans its grid
    hipLaunchKernelGGL(wsum_kernel, dim3(N), dim3(64), 0, st, w, w_per_sample, N, C, wsum);
    hipLaunchKernelGGL(whmse_kernel, grid, dim3(256), 0, st, v3(s), v3(t), m3(grad), w, w_per_sample, (const float *)wsum,
                       grad_scale, N, C, (long long)P, sel.per_chunk, partial);
    KD_CHECK_LAUNCH("kd_weighted_hint_mse");
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(256), 0, st, (const double *)partial, sel.blocks, 1.0 / (double)N,
                       (const double *)nullptr, loss);
    KD_CHECK_LAUNCH("kd_weighted_hint_mse(finish)");
    return KD_OK;
}

// ---- kd_ce2d / kd_ce2d_weighted and their gradient ----------------------------------------------------------------------------------
static int ce2d_impl(const char *who, const kd_view3 *x, const int64_t *target, const float *class_weight, int32_t sum_reduction, int32_t ignore_index,
                     int32_t N, int32_t C, int64_t P, float *loss, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    KD_REQUIRE(x && x->ptr && target && loss && workspace, KD_ERR_INVALID, "%s: null argument", who);
    KD_REQUIRE(ok_dt(x->dtype) && N > 0 && C > 0 && P > 0, KD_ERR_INVALID, "%s: bad argument", who);
    KD_REQUIRE(workspace_bytes >= kd_loss_workspace(N, C, P), KD_ERR_WORKSPACE, "%s: workspace too small", who);
    double *partial = (double *)workspace, *count = partial + LOSS_MAX_BLOCKS;
    hipStream_t st = (hipStream_t)stream;
    const LossSel sel = loss_select_ce2d(x, N, C, P);
    KD_NOTE_PLUMBING(loss_kernel_name(sel.kernel));
    auto nhwc = [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(ce2d_nhwc_kernel<T>, dim3(sel.blocks), dim3(256), sel.lds, st, (const T *)x->ptr, target, ignore_index, C,
                           (long long)N * P, partial, count, class_weight);
    };
    switch (sel.kernel) {
    case LK_CE2D_NHWC_F32: nhwc(float{}); break;
    case LK_CE2D_NHWC_BF16: nhwc(bf16_t{}); break;
    case LK_CE2D:
        hipLaunchKernelGGL(ce2d_kernel, dim3(sel.blocks), dim3(256), 0, st, v3(x), target, ignore_index, N, C, (long long)P, partial, count, class_weight);
        break;
    default: return no_launch(who, sel);
    }
    KD_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(256), 0, st, (const double *)partial, sel.blocks, 1.0,
                       sum_reduction ? (const double *)nullptr : (const double *)count, loss);
    KD_CHECK_LAUNCH(who);
    return KD_OK;
}

extern "C" int kd_ce2d(const kd_view3 *x, const int64_t *target, int32_t ignore_index, int32_t N, int32_t C, int64_t P,
                       float *loss, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    return ce2d_impl("kd_ce2d", x, target, nullptr, 0, ignore_index, N, C, P, loss, workspace, workspace_bytes, stream);
}

extern "C" int kd_ce2d_weighted(const kd_view3 *x, const int64_t *target, const float *class_weight, int32_t sum_reduction, int32_t ignore_index,
                                int32_t N, int32_t C, int64_t P, float *loss, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    return ce2d_impl("kd_ce2d_weighted", x, target, class_weight, sum_reduction, ignore_index, N, C, P, loss, workspace, workspace_bytes, stream);
}

static int ce2d_grad_impl(const char *who, const kd_view3 *x, const int64_t *target, const float *class_weight, int32_t sum_reduction, int32_t ignore_index,
                          int32_t N, int32_t C, int64_t P, const kd_mview3 *grad, float grad_scale, void *workspace, size_t workspace_bytes,
                          kd_stream_t stream)
{
    KD_REQUIRE(x && x->ptr && target && grad && grad->ptr && workspace, KD_ERR_INVALID, "%s: null argument", who);
    KD_REQUIRE(ok_dt(x->dtype) && ok_dt(grad->dtype) && N > 0 && C > 0 && P > 0, KD_ERR_INVALID, "%s: bad argument", who);
    KD_REQUIRE(workspace_bytes >= kd_loss_workspace(N, C, P), KD_ERR_WORKSPACE, "%s: workspace too small", who);
    double *count = (double *)workspace;
    const LossSel sel = loss_flat(LK_CE2D_GRAD, (long long)N * P);
    hipStream_t st = (hipStream_t)stream;
    KD_NOTE_PLUMBING(loss_kernel_name(sel.kernel));
    hipLaunchKernelGGL(ce2d_count_kernel, dim3(sel.blocks), dim3(256), 0, st, target, ignore_index, C, (long long)N * P, count, class_weight);
    KD_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(ce2d_grad_kernel, dim3(sel.blocks), dim3(256), 0, st, v3(x), target, ignore_index, N, C, (long long)P, m3(grad), grad_scale,
                       (const double *)count, sel.blocks, class_weight, (int)sum_reduction);
    KD_CHECK_LAUNCH(who);
    return KD_OK;
}

extern "C" int kd_ce2d_grad(const kd_view3 *x, const int64_t *target, int32_t ignore_index, int32_t N, int32_t C, int64_t P,
                            const kd_mview3 *grad, float grad_scale, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    return ce2d_grad_impl("kd_ce2d_grad", x, target, nullptr, 0, ignore_index, N, C, P, grad, grad_scale, workspace, workspace_bytes, stream);
}

extern "C" int kd_ce2d_weighted_grad(const kd_view3 *x, const int64_t *target, const float *class_weight, int32_t sum_reduction, int32_t ignore_index,
                                     int32_t N, int32_t C, int64_t P, const kd_mview3 *grad, float grad_scale, void *workspace,
                                     size_t workspace_bytes, kd_stream_t stream)
{
    return ce2d_grad_impl("kd_ce2d_weighted_grad", x, target, class_weight, sum_reduction, ignore_index, N, C, P, grad, grad_scale, workspace,
                          workspace_bytes, stream);
}

extern "C" int kd_confusion(const kd_view3 *x, const int64_t *target, int32_t N, int32_t C, int64_t P, int64_t *conf,
                            int32_t accumulate, kd_stream_t stream)
{
    KD_REQUIRE(x && x->ptr && target && conf, KD_ERR_INVALID, "kd_confusion: null argument");
    KD_REQUIRE(ok_dt(x->dtype) && N > 0 && P > 0, KD_ERR_INVALID, "kd_confusion: bad argument");
    KD_REQUIRE(C >= 1 && C <= 64, KD_ERR_UNSUPPORTED, "kd_confusion: 1 <= C <= 64 classes (got %d)", C);
    KD_REQUIRE(((uintptr_t)conf & 7) == 0, KD_ERR_INVALID, "kd_confusion: conf must be 8-B aligned");
    hipStream_t st = (hipStream_t)stream;
    if (!accumulate) {
        if (hipMemsetAsync(conf, 0, (size_t)C * C * sizeof(int64_t), st) != hipSuccess) {
            kd_set_error("kd_confusion: hipMemsetAsync failed");
            return KD_ERR_HIP;
        }
    }
    const LossSel sel = loss_select_confusion(x, N, C, P);
    KD_NOTE_PLUMBING(loss_kernel_name(sel.kernel));
    auto nhwc = [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(confusion_nhwc_kernel<T>, dim3(sel.blocks), dim3(256), sel.lds, st, (const T *)x->ptr, target, C, (long long)N * P,
                           (unsigned long long *)conf);
    };
    switch (sel.kernel) {
    case LK_CONFUSION_NHWC_F32: nhwc(float{}); break;
    case LK_CONFUSION_NHWC_BF16: nhwc(bf16_t{}); break;
    case LK_CONFUSION:
        hipLaunchKernelGGL(confusion_kernel, dim3(sel.blocks), dim3(256), sel.lds, st, v3(x), target, N, C, (long long)P, (unsigned long long *)conf);
        break;
    default: return no_launch("kd_confusion", sel);
    }
    KD_CHECK_LAUNCH("kd_confusion");
    return KD_OK;
}

// ---- kd_ce2d_up / kd_kldiv_up / kd_jsdiv_up / kd_focal_up / kd_logit_metrics_up: from the low-resolution logits (see ce2d_up_kernel) ----
// Each asks loss_select_up right after its null checks (the selector is total) and reports a class count above its bound where it
// always has, with its own message.  What the five share after their own argument checks is here: the workspace and
// resampling-ratio checks and the geometry the kernels take.  say_scale: the ratio message names the scale.
static int up_plan(UpGeom &g, const LossSel &sel, const char *who, bool say_scale, int32_t N, int32_t h, int32_t w, int32_t C, int32_t H, int32_t W,
                   size_t workspace_bytes)
{
    KD_REQUIRE(workspace_bytes >= kd_loss_workspace(N, C, (int64_t)H * W), KD_ERR_WORKSPACE, "%s: workspace too small", who);
    if (sel.why == LOSS_WHY_SPAN) {
        if (say_scale)
            kd_set_error("%s: a 256-pixel chunk spans more than %d source columns (scale %dx%d -> %dx%d): materialise the logits", who, LOSS_UP_NW, h, w, H, W);
        else
            kd_set_error("%s: a 256-pixel chunk spans more than %d source columns: materialise the logits", who, LOSS_UP_NW);
        return KD_ERR_UNSUPPORTED;
    }
    KD_REQUIRE(sel.kernel != LOSS_REFUSED, KD_ERR_UNSUPPORTED, "%s: no kernel selected", who);
    g = UpGeom{N, h, w, C, H, W, sel.sh, sel.sw, sel.oh, sel.ow};
    return KD_OK;
}

extern "C" int kd_ce2d_up(const float *x_lo, const int64_t *target, int32_t ignore_index, int32_t N, int32_t h, int32_t w, int32_t C,
                          int32_t H, int32_t W, int32_t align_corners, float *loss, void *workspace, size_t workspace_bytes,
                          kd_stream_t stream)
{
    KD_REQUIRE(x_lo && target && loss && workspace, KD_ERR_INVALID, "kd_ce2d_up: null argument");
    const LossSel sel = loss_select_up(LOSS_UP_CE2D, N, h, w, C, H, W, align_corners);
    KD_REQUIRE(N > 0 && h > 0 && w > 0 && C > 0 && sel.why != LOSS_WHY_CLASSES && H > 0 && W > 0, KD_ERR_INVALID, "kd_ce2d_up: bad argument (C <= 48: the staged patch fits 64 KiB of LDS)");
    UpGeom g;
    if (const int rc = up_plan(g, sel, "kd_ce2d_up", true, N, h, w, C, H, W, workspace_bytes)) return rc;
    double *partial = (double *)workspace, *count = partial + LOSS_MAX_BLOCKS;
    hipStream_t st = (hipStream_t)stream;
    KD_NOTE_PLUMBING(loss_kernel_name(sel.kernel));
    auto fn = launch_of(sel.kernel, LK_CE2D_UP_19, ce2d_up_kernel<19>, LK_CE2D_UP_0, ce2d_up_kernel<0>);
    if (!fn) return no_launch("kd_ce2d_up", sel);
    hipLaunchKernelGGL(fn, dim3(sel.blocks), dim3(256), sel.lds, st, x_lo, target, ignore_index, g, sel.nchunks, sel.cpr, partial, count);
    KD_CHECK_LAUNCH("kd_ce2d_up");
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(256), 0, st, (const double *)partial, sel.blocks, 1.0, (const double *)count, loss);
    KD_CHECK_LAUNCH("kd_ce2d_up(finish)");
    return KD_OK;
}

// kd_kldiv_up / kd_jsdiv_up: the same call on the kernel of their kind; loss_scale as kd_kldiv / kd_jsdiv
static int pair_up_impl(const char *who, const char *who_finish, LossUpOp op, const float *s_lo, const float *t_lo, float temperature, int32_t N, int32_t h, int32_t w, int32_t C,
                        int32_t H, int32_t W, int32_t align_corners, float *loss, double loss_scale, void *workspace, size_t workspace_bytes,
                        kd_stream_t stream)
{
    KD_REQUIRE(s_lo && t_lo && loss && workspace, KD_ERR_INVALID, "%s: null argument", who);
    const LossSel sel = loss_select_up(op, N, h, w, C, H, W, align_corners);
    KD_REQUIRE(N > 0 && h > 0 && w > 0 && C > 0 && sel.why != LOSS_WHY_CLASSES && H > 0 && W > 0 && temperature > 0.f, KD_ERR_INVALID,
               "%s: bad argument (C <= 24: two staged patches fit 64 KiB of LDS)", who);
    UpGeom g;
    if (const int rc = up_plan(g, sel, who, false, N, h, w, C, H, W, workspace_bytes)) return rc;
    double *partial = (double *)workspace;
    hipStream_t st = (hipStream_t)stream;
    KD_NOTE_PLUMBING(loss_kernel_name(sel.kernel));
    auto fn = launch_of(sel.kernel, LK_KLDIV_UP_19, pair_up_kernel<PAIR_KLD, 19>, LK_KLDIV_UP_0, pair_up_kernel<PAIR_KLD, 0>, LK_JSDIV_UP_19,
                        pair_up_kernel<PAIR_JSD, 19>, LK_JSDIV_UP_0, pair_up_kernel<PAIR_JSD, 0>);
    if (!fn) return no_launch(who, sel);
    hipLaunchKernelGGL(fn, dim3(sel.blocks), dim3(256), sel.lds, st, s_lo, t_lo, g, 1.f / temperature, sel.nchunks, sel.cpr, partial);
    KD_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(256), 0, st, (const double *)partial, sel.blocks, loss_scale, (const double *)nullptr, loss);
    KD_CHECK_LAUNCH(who_finish);
    return KD_OK;
}

extern "C" int kd_kldiv_up(const float *s_lo, const float *t_lo, float temperature, int32_t N, int32_t h, int32_t w, int32_t C, int32_t H,
                           int32_t W, int32_t align_corners, float *loss, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    // 'mean' over N*C*P elements, then * T^2 * C  ==  T^2 / (N*P) * sum  (kd_kldiv)
    const double scale = (double)temperature * temperature / ((double)N * (double)H * (double)W);
    return pair_up_impl("kd_kldiv_up", "kd_kldiv_up(finish)", LOSS_UP_KLDIV, s_lo, t_lo, temperature, N, h, w, C, H, W, align_corners, loss, scale, workspace, workspace_bytes, stream);
}

extern "C" int kd_jsdiv_up(const float *s_lo, const float *t_lo, float temperature, int32_t N, int32_t h, int32_t w, int32_t C, int32_t H,
                           int32_t W, int32_t align_corners, float *loss, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    // T^2 / (2N) * sum  (kd_jsdiv)
    const double scale = (double)temperature * temperature / (2.0 * (double)N);
    return pair_up_impl("kd_jsdiv_up", "kd_jsdiv_up(finish)", LOSS_UP_JSDIV, s_lo, t_lo, temperature, N, h, w, C, H, W, align_corners, loss, scale, workspace, workspace_bytes, stream);
}

extern "C" int kd_logit_metrics_up(const float *s_lo, const float *t_lo, const int64_t *target, int32_t ignore_index, int32_t N, int32_t h,
                                   int32_t w, int32_t C, int32_t H, int32_t W, int32_t align_corners, float *out, int64_t *conf_s,
                                   int64_t *conf_t, int32_t accumulate, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    KD_REQUIRE(s_lo && t_lo && target && out && conf_s && conf_t && workspace, KD_ERR_INVALID, "kd_logit_metrics_up: null argument");
    KD_REQUIRE(N > 0 && h > 0 && w > 0 && C > 0 && H > 0 && W > 0, KD_ERR_INVALID, "kd_logit_metrics_up: bad argument");
    KD_REQUIRE(conf_s != conf_t && (((uintptr_t)conf_s | (uintptr_t)conf_t | (uintptr_t)workspace) & 7) == 0, KD_ERR_INVALID,
               "kd_logit_metrics_up: conf_s / conf_t must be two 8-B aligned matrices, the workspace 8-B aligned");
    const LossSel sel = loss_select_up(LOSS_UP_METRICS, N, h, w, C, H, W, align_corners);
    KD_REQUIRE(sel.why != LOSS_WHY_CLASSES, KD_ERR_UNSUPPORTED, "kd_logit_metrics_up: C <= 48 (got %d): materialise the logits", C);
    UpGeom g;
    if (const int rc = up_plan(g, sel, "kd_logit_metrics_up", true, N, h, w, C, H, W, workspace_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (!accumulate) {
        if (hipMemsetAsync(conf_s, 0, (size_t)C * C * sizeof(int64_t), st) != hipSuccess ||
            hipMemsetAsync(conf_t, 0, (size_t)C * C * sizeof(int64_t), st) != hipSuccess) {
            kd_set_error("kd_logit_metrics_up: hipMemsetAsync failed");
            return KD_ERR_HIP;
        }
    }
    double *partial = (double *)workspace;
    auto fn = launch_of(sel.kernel, LK_METRICS_UP_19, logit_metrics_up_kernel<19>, LK_METRICS_UP_0, logit_metrics_up_kernel<0>);
    if (!fn) return no_launch("kd_logit_metrics_up", sel);
    // two staged patches + two C x C histograms: 50.3 KiB at 19 classes, 138 KiB at 48 (of the CU's 160 KiB)
    if (sel.lds > LOSS_LDS_DEFAULT) {
        if (hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sel.lds) != hipSuccess) {
            (void)hipGetLastError();
            kd_set_error("kd_logit_metrics_up: cannot reserve %zu B of LDS", sel.lds);
            return KD_ERR_UNSUPPORTED;
        }
    }
    KD_NOTE_PLUMBING(loss_kernel_name(sel.kernel));
    hipLaunchKernelGGL(fn, dim3(sel.blocks), dim3(256), sel.lds, st, s_lo, t_lo, target, ignore_index, g, sel.nchunks, sel.cpr, partial,
                       (unsigned long long *)conf_s, (unsigned long long *)conf_t);
    KD_CHECK_LAUNCH("kd_logit_metrics_up");
    hipLaunchKernelGGL(logit_metrics_finish_kernel, dim3(1), dim3(256), 0, st, (const double *)partial, sel.blocks,
                       1.0 / ((double)N * (double)C * (double)H * (double)W), out);
    KD_CHECK_LAUNCH("kd_logit_metrics_up(finish)");
    return KD_OK;
}

// ---- kd_kldiv_multi / kd_softmax_mean ---------------------------------------------------------------------------------------
namespace {
// the targets by value, weights divided by their sum; false (error set) on a bad argument
bool mt_pack(const char *who, const kd_multi_targets *ts, MT &mt)
{
    if (!ts || ts->n < 1 || ts->n > KD_MULTI_MAX) {
        kd_set_error("%s: 1 to %d operands, got %d", who, KD_MULTI_MAX, ts ? (int)ts->n : 0);
        return false;
    }
    double W = 0.0;
    for (int k = 0; k < ts->n; ++k) {
        if (!ts->t[k].ptr || !ok_dt(ts->t[k].dtype) || !(ts->w[k] >= 0.f)) {
            kd_set_error("%s: operand %d: null pointer, bad dtype or negative weight", who, k);
            return false;
        }
        W += (double)ts->w[k];
    }
    if (!(W > 0.0) || W > 3.0e38) {
        kd_set_error("%s: the weights must have a positive finite sum", who);
        return false;
    }
    mt.n = ts->n;
    for (int k = 0; k < KD_MULTI_MAX; ++k) {
        mt.t[k] = k < ts->n ? v3(&ts->t[k]) : V3{nullptr, 0, 0, 0, 0};
        mt.w[k] = k < ts->n ? (float)((double)ts->w[k] / W) : 0.f;
    }
    return true;
}
}  // namespace

// Both entry points launch through this; kd_softmax_mean has no student, labels, scales or partials.
static int multi_launch(const char *who, const LossSel &sel, hipStream_t st, V3 sv, const MT &mt, M3 gv, const int64_t *labels, int ignore_index,
                        float invT, float gk, float sup_scale, int C, long long P, long long rows, const double *cnt, int ncount, double *pkd,
                        double *pce)
{
    KD_NOTE_PLUMBING(loss_kernel_name(sel.kernel));
    if (sel.kernel == LK_KLDM_NHWC) {
        hipLaunchKernelGGL(kldm_nhwc_kernel, dim3(sel.blocks), dim3(256), sel.lds, st, sv, mt, gv, labels, ignore_index, invT, gk, sup_scale, C, rows,
                           cnt, ncount, pkd, pce);
    } else {
        auto fn = launch_of(sel.kernel, LK_MT_WAVE_1_VEC, mt_wave_kernel<1, true, false>, LK_MT_WAVE_1_NOVEC, mt_wave_kernel<1, false, false>,
                            LK_MT_WAVE_4_VEC, mt_wave_kernel<4, true, false>, LK_MT_WAVE_4_NOVEC, mt_wave_kernel<4, false, false>,
                            LK_SM_WAVE_1_VEC, mt_wave_kernel<1, true, true>, LK_SM_WAVE_1_NOVEC, mt_wave_kernel<1, false, true>,
                            LK_SM_WAVE_4_VEC, mt_wave_kernel<4, true, true>, LK_SM_WAVE_4_NOVEC, mt_wave_kernel<4, false, true>,
                            LK_KLDM, kldm_kernel<false>, LK_KLDM_SMEAN, kldm_kernel<true>);
        if (!fn) return no_launch(who, sel);
        hipLaunchKernelGGL(fn, dim3(sel.blocks), dim3(256), 0, st, sv, mt, gv, labels, ignore_index, invT, gk, sup_scale, C, P, rows, cnt, ncount, pkd, pce);
    }
    KD_CHECK_LAUNCH(who);
    return KD_OK;
}

extern "C" int kd_kldiv_multi(const kd_view3 *s, const kd_multi_targets *targets, float temperature, const int64_t *labels,
                              int32_t ignore_index, float kd_scale, float sup_scale, int32_t N, int32_t C, int64_t P, float *losses,
                              const kd_mview3 *grad, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    KD_REQUIRE(s && s->ptr && losses && workspace, KD_ERR_INVALID, "kd_kldiv_multi: null argument");
    KD_REQUIRE(ok_dt(s->dtype) && (!grad || (grad->ptr && ok_dt(grad->dtype))), KD_ERR_INVALID, "kd_kldiv_multi: bad dtype");
    KD_REQUIRE(N > 0 && C > 0 && P > 0, KD_ERR_INVALID, "kd_kldiv_multi: bad shape");
    KD_REQUIRE(temperature > 0.f, KD_ERR_INVALID, "kd_kldiv_multi: temperature must be positive");
    KD_REQUIRE(workspace_bytes >= kd_loss_workspace(N, C, P), KD_ERR_WORKSPACE, "kd_kldiv_multi: workspace too small");
    KD_REQUIRE(((uintptr_t)workspace & 7) == 0, KD_ERR_INVALID, "kd_kldiv_multi: workspace must be 8-B aligned");
    MT mt;
    if (!mt_pack("kd_kldiv_multi", targets, mt)) return KD_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    double *pkd = (double *)workspace, *pce = pkd + LOSS_MT_MAX_BLOCKS, *count = pce + LOSS_MT_MAX_BLOCKS;
    const long long rows = (long long)N * P;
    const LossSel sel = loss_select_multi(s, targets, grad, false, N, C, P);
    const float gk = kd_scale * temperature / ((float)N * (float)P);
    int ncount = 0;
    if (labels) {
        ncount = loss_blocks_for(rows, LOSS_MT_MAX_BLOCKS);
        hipLaunchKernelGGL(ce2d_count_kernel, dim3(ncount), dim3(256), 0, st, labels, ignore_index, C, rows, count, (const float *)nullptr);
        KD_CHECK_LAUNCH("kd_kldiv_multi(count)");
    }
    const double *cnt = labels ? count : nullptr;
    if (const int rc = multi_launch("kd_kldiv_multi", sel, st, v3(s), mt, m3(grad), labels, ignore_index, 1.f / temperature, gk, sup_scale, C, P, rows,
                                    cnt, ncount, pkd, pce))
        return rc;
    // per target 'mean' over N*C*P elements, then * T^2 * C  ==  T^2 / (N*P) * sum; the weights already sum to 1
    const double kd_mul = (double)temperature * temperature / ((double)N * (double)P);
    hipLaunchKernelGGL(mt_finish_kernel, dim3(1), dim3(256), 0, st, (const double *)pkd, (const double *)pce, sel.blocks, cnt, ncount, kd_mul,
                       kd_scale, sup_scale, losses);
    KD_CHECK_LAUNCH("kd_kldiv_multi(finish)");
    return KD_OK;
}

extern "C" int kd_softmax_mean(const kd_multi_targets *logits, float temperature, int32_t N, int32_t C, int64_t P, const kd_mview3 *out,
                               kd_stream_t stream)
{
    KD_REQUIRE(out && out->ptr && out->dtype == KD_F32, KD_ERR_INVALID, "kd_softmax_mean: out must be an fp32 view");
    KD_REQUIRE(N > 0 && C > 0 && P > 0, KD_ERR_INVALID, "kd_softmax_mean: bad shape");
    KD_REQUIRE(temperature > 0.f, KD_ERR_INVALID, "kd_softmax_mean: temperature must be positive");
    MT mt;
    if (!mt_pack("kd_softmax_mean", logits, mt)) return KD_ERR_INVALID;
    const LossSel sel = loss_select_multi(nullptr, logits, out, true, N, C, P);
    return multi_launch("kd_softmax_mean", sel, (hipStream_t)stream, V3{nullptr, 0, 0, 0, 0}, mt, m3(out), nullptr, 0, 1.f / temperature, 0.f, 0.f, C, P,
                        (long long)N * P, nullptr, 0, nullptr, nullptr);
}

// ---- kd_focal / kd_focal_grad / kd_focal_up -----------------------------------------------------------------------------------------
extern "C" int kd_focal(const kd_view3 *x, const int64_t *target, const float *alpha, float gamma, int32_t ignore_index, int32_t reduction,
                        int32_t N, int32_t C, int64_t P, float *loss, double *stats, float *a_map, float *ce_map, void *workspace,
                        size_t workspace_bytes, kd_stream_t stream)
{
    KD_REQUIRE(x && x->ptr && target && workspace, KD_ERR_INVALID, "kd_focal: null argument");
    KD_REQUIRE(ok_dt(x->dtype) && N > 0 && C > 0 && P > 0 && gamma >= 0.f, KD_ERR_INVALID, "kd_focal: bad argument");
    KD_REQUIRE(reduction >= 0 && reduction <= 2, KD_ERR_INVALID, "kd_focal: reduction is 0 (none), 1 (mean) or 2 (sum)");
    KD_REQUIRE(reduction == 0 || loss, KD_ERR_INVALID, "kd_focal: 'mean' / 'sum' need a loss pointer");
    KD_REQUIRE(reduction != 0 || (a_map && ce_map), KD_ERR_INVALID, "kd_focal: 'none' needs both per-pixel maps");
    KD_REQUIRE((a_map == nullptr) == (ce_map == nullptr), KD_ERR_INVALID, "kd_focal: a_map and ce_map go together");
    KD_REQUIRE(workspace_bytes >= kd_loss_workspace(N, C, P), KD_ERR_WORKSPACE, "kd_focal: workspace too small");
    KD_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)stats & 7) == 0, KD_ERR_INVALID, "kd_focal: workspace / stats must be 8-B aligned");
    double *partial = (double *)workspace;
    const long long total = (long long)N * P;
    const LossSel sel = loss_flat(LK_FOCAL, total, LOSS_FOCAL_MAX_BLOCKS);
    hipStream_t st = (hipStream_t)stream;
    KD_NOTE_PLUMBING(loss_kernel_name(sel.kernel));
    hipLaunchKernelGGL(focal_kernel, dim3(sel.blocks), dim3(256), 0, st, v3(x), target, alpha, gamma, ignore_index, N, C, (long long)P, a_map, ce_map, partial);
    KD_CHECK_LAUNCH("kd_focal");
    hipLaunchKernelGGL(focal_finish_kernel, dim3(1), dim3(256), 0, st, (const double *)partial, sel.blocks, (int)reduction, (double)total, stats,
                       reduction == 0 ? (float *)nullptr : loss);
    KD_CHECK_LAUNCH("kd_focal(finish)");
    return KD_OK;
}

extern "C" int kd_focal_grad(const kd_view3 *x, const int64_t *target, const float *alpha, float gamma, int32_t ignore_index, int32_t reduction,
                             int32_t N, int32_t C, int64_t P, const double *stats, const float *upstream, const float *a_map,
                             const float *ce_map, const kd_mview3 *grad, kd_stream_t stream)
{
    KD_REQUIRE(x && x->ptr && target && upstream && grad && grad->ptr, KD_ERR_INVALID, "kd_focal_grad: null argument");
    KD_REQUIRE(ok_dt(x->dtype) && ok_dt(grad->dtype) && N > 0 && C > 0 && P > 0 && gamma >= 0.f, KD_ERR_INVALID, "kd_focal_grad: bad argument");
    KD_REQUIRE(reduction >= 0 && reduction <= 2, KD_ERR_INVALID, "kd_focal_grad: reduction is 0 (none), 1 (mean) or 2 (sum)");
    KD_REQUIRE(reduction == 0 ? (a_map && ce_map) : stats != nullptr, KD_ERR_INVALID,
               "kd_focal_grad: 'none' needs the forward's per-pixel maps, 'mean' / 'sum' its stats");
    const LossSel sel = loss_flat(LK_FOCAL_GRAD, (long long)N * P);
    KD_NOTE_PLUMBING(loss_kernel_name(sel.kernel));
    hipLaunchKernelGGL(focal_grad_kernel, dim3(sel.blocks), dim3(256), 0, (hipStream_t)stream, v3(x), target, alpha, gamma,
                       ignore_index, (int)reduction, N, C, (long long)P, stats, upstream, a_map, ce_map, m3(grad));
    KD_CHECK_LAUNCH("kd_focal_grad");
    return KD_OK;
}

extern "C" int kd_focal_up(const float *x_lo, const int64_t *target, const float *alpha, float gamma, int32_t ignore_index, int32_t reduction,
                           int32_t N, int32_t h, int32_t w, int32_t C, int32_t H, int32_t W, int32_t align_corners, float *loss, double *stats,
                           void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    KD_REQUIRE(x_lo && target && loss && workspace, KD_ERR_INVALID, "kd_focal_up: null argument");
    const LossSel sel = loss_select_up(LOSS_UP_FOCAL, N, h, w, C, H, W, align_corners);
    KD_REQUIRE(N > 0 && h > 0 && w > 0 && C > 0 && sel.why != LOSS_WHY_CLASSES && H > 0 && W > 0 && gamma >= 0.f, KD_ERR_INVALID,
               "kd_focal_up: bad argument (C <= 48: the staged patch fits 64 KiB of LDS)");
    KD_REQUIRE(reduction == 1 || reduction == 2, KD_ERR_INVALID, "kd_focal_up: reduction is 1 (mean) or 2 (sum)");
    // (the size before the alignment, as this entry point always reported them; up_plan repeats the size check)
    KD_REQUIRE(workspace_bytes >= kd_loss_workspace(N, C, (int64_t)H * W), KD_ERR_WORKSPACE, "kd_focal_up: workspace too small");
    KD_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)stats & 7) == 0, KD_ERR_INVALID, "kd_focal_up: workspace / stats must be 8-B aligned");
    UpGeom g;
    if (const int rc = up_plan(g, sel, "kd_focal_up", false, N, h, w, C, H, W, workspace_bytes)) return rc;
    double *partial = (double *)workspace;
    hipStream_t st = (hipStream_t)stream;
    KD_NOTE_PLUMBING(loss_kernel_name(sel.kernel));
    auto fn = launch_of(sel.kernel, LK_FOCAL_UP_19, focal_up_kernel<19>, LK_FOCAL_UP_0, focal_up_kernel<0>);
    if (!fn) return no_launch("kd_focal_up", sel);
    hipLaunchKernelGGL(fn, dim3(sel.blocks), dim3(256), sel.lds, st, x_lo, target, alpha, gamma, ignore_index, g, sel.nchunks, sel.cpr, partial);
    KD_CHECK_LAUNCH("kd_focal_up");
    hipLaunchKernelGGL(focal_finish_kernel, dim3(1), dim3(256), 0, st, (const double *)partial, sel.blocks, (int)reduction, (double)N * H * W, stats, loss);
    KD_CHECK_LAUNCH("kd_focal_up(finish)");
    return KD_OK;
}

// ---- kd_topk_hint_mse ------------------------------------------------------------------------------------------------------------
extern "C" size_t kd_topk_hint_workspace(int32_t N, int32_t C, int64_t P) { return loss_topk_workspace_bytes(N, C, P); }

extern "C" int kd_topk_hint_mse(const kd_view3 *s, const kd_view3 *t, int32_t K, int32_t N, int32_t C, int64_t P, float *loss,
                                const kd_mview3 *grad, float grad_scale, float *mask, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    KD_REQUIRE(s && t && s->ptr && t->ptr && loss && workspace, KD_ERR_INVALID, "kd_topk_hint_mse: null argument");
    KD_REQUIRE(ok_dt(s->dtype) && ok_dt(t->dtype) && (!grad || ok_dt(grad->dtype)), KD_ERR_INVALID, "kd_topk_hint_mse: bad dtype");
    KD_REQUIRE(N > 0 && C > 0 && P > 0, KD_ERR_INVALID, "kd_topk_hint_mse: bad shape");
    KD_REQUIRE(K >= 1 && K <= C, KD_ERR_INVALID, "kd_topk_hint_mse: K = %d channels kept of %d: need 1 <= K <= C", K, C);
    const LossSel sel = loss_select_topk(s, t, grad, mask, workspace, N, C, P);
    KD_REQUIRE(sel.why != LOSS_WHY_TOPK_MAX_C, KD_ERR_UNSUPPORTED, "kd_topk_hint_mse: C = %d > %d channels", C, LOSS_TOPK_MAX_C);
    KD_REQUIRE(workspace_bytes >= kd_topk_hint_workspace(N, C, P), KD_ERR_WORKSPACE, "kd_topk_hint_mse: workspace too small");
    KD_REQUIRE(((uintptr_t)workspace & 7) == 0, KD_ERR_INVALID, "kd_topk_hint_mse: workspace must be 8-B aligned");
    const int nchunk = sel.chunks;
    const size_t nc = (size_t)N * C;
    double *pt2 = (double *)workspace, *pd2 = pt2 + nc * nchunk, *part = pd2 + nc * nchunk;
    float *mk = mask ? mask : (float *)((char *)workspace + sel.aux_off);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(topk_sums_kernel, dim3((unsigned)nchunk, (unsigned)((C + 63) / 64), (unsigned)N), dim3(256), 0, st, v3(s), v3(t), C,
                       (long long)P, sel.per_chunk, nchunk, pt2, pd2);
    KD_CHECK_LAUNCH("kd_topk_hint_mse(sums)");
    hipLaunchKernelGGL(topk_select_kernel, dim3(N), dim3(1024), (size_t)C * sizeof(double), st, (const double *)pt2, (const double *)pd2, C,
                       nchunk, (int)K, mk, part);
    KD_CHECK_LAUNCH("kd_topk_hint_mse(select)");
    // loss = sum_n sum_kept mean_p (s-t)^2 / (N K) ; grad = 2 mask (s-t) / (P N K)
    const double denom = (double)N * (double)K;
    const float gscale = (float)((double)grad_scale * 2.0 / ((double)P * denom));
    const long long numel = (long long)nc * P;
    KD_NOTE_PLUMBING(loss_kernel_name(sel.kernel));
    auto vec = [&](auto z, auto cfast) {
        using T = decltype(z);
        hipLaunchKernelGGL((topk_grad_vec_kernel<T, decltype(cfast)::value>), dim3(sel.blocks), dim3(256), 0, st, (const T *)s->ptr,
                           (const T *)t->ptr, (T *)grad->ptr, (const float *)mk, gscale, C, (long long)P, numel / 8);
    };
    switch (sel.kernel) {
    case LK_TOPK_VEC_F32_CFAST: vec(float{}, std::true_type{}); break;
    case LK_TOPK_VEC_F32_PFAST: vec(float{}, std::false_type{}); break;
    case LK_TOPK_VEC_BF16_CFAST: vec(bf16_t{}, std::true_type{}); break;
    case LK_TOPK_VEC_BF16_PFAST: vec(bf16_t{}, std::false_type{}); break;
    case LK_TOPK_GRAD:
        hipLaunchKernelGGL(topk_grad_kernel, dim3(sel.blocks), dim3(256), 0, st, v3(s), v3(t), m3(grad), (const float *)mk, gscale, N, C, (long long)P,
                           s->sC == 1 ? 1 : 0);
        break;
    case LK_TOPK_NOGRAD: break;     // no gradient asked for: the sums, the selection and the loss alone
    default: return no_launch("kd_topk_hint_mse", sel);
    }
    if (sel.kernel != LK_TOPK_NOGRAD) KD_CHECK_LAUNCH("kd_topk_hint_mse(grad)");
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(256), 0, st, (const double *)part, (int)N, 1.0 / ((double)P * denom), (const double *)nullptr, loss);
    KD_CHECK_LAUNCH("kd_topk_hint_mse(finish)");
    return KD_OK;
}

// ---- kd_radam_step / kd_radam_step_multi / kd_scale_by_device_scalar ---------------------------------------------------------------
// (N_sma, step_size) exactly as utils/optim/radam.py:64-83 computes (and caches) them
static void radam_constants(int step, float beta1, float beta2, int *rect, double *step_size)
{
    const double beta2_t = pow((double)beta2, step);
    const double nmax = 2.0 / (1.0 - (double)beta2) - 1.0;
    const double nsma = nmax - 2.0 * step * beta2_t / (1.0 - beta2_t);
    *rect = nsma >= 5.0;
    if (*rect)
        *step_size = sqrt((1 - beta2_t) * (nsma - 4) / (nmax - 4) * (nsma - 2) / nsma * nmax / (nmax - 2)) / (1 - pow((double)beta1, step));
    else
        *step_size = 1.0 / (1 - pow((double)beta1, step));
}

extern "C" int kd_radam_step(float *p, const float *g, float *exp_avg, float *exp_avg_sq, int64_t n, int32_t step, float lr,
                             float beta1, float beta2, float eps, float weight_decay, kd_stream_t stream)
{
    KD_REQUIRE(p && g && exp_avg && exp_avg_sq && n > 0 && step >= 1, KD_ERR_INVALID, "kd_radam_step: bad argument");
    int rect;
    double step_size;
    radam_constants(step, beta1, beta2, &rect, &step_size);
    const LossSel sel = loss_flat(LK_RADAM, n);
    KD_NOTE_PLUMBING(loss_kernel_name(sel.kernel));
    hipLaunchKernelGGL(radam_kernel, dim3(sel.blocks), dim3(256), 0, (hipStream_t)stream, p, g, exp_avg, exp_avg_sq,
                       (long long)n, beta1, beta2, eps, (float)((double)weight_decay * lr), (float)(step_size * lr), rect);
    KD_CHECK_LAUNCH("kd_radam_step");
    return KD_OK;
}

extern "C" int kd_scale_by_device_scalar(void *x, int32_t dtype, int64_t n, const float *scale, kd_stream_t stream)
{
    KD_REQUIRE(x && scale && n > 0, KD_ERR_INVALID, "kd_scale_by_device_scalar: bad argument");
    KD_REQUIRE(dtype == KD_F32 || dtype == KD_BF16, KD_ERR_INVALID, "kd_scale_by_device_scalar: bad dtype");
    KD_REQUIRE(kd_aligned16(x), KD_ERR_INVALID, "kd_scale_by_device_scalar: x must be 16-B aligned");
    const LossSel sel = loss_select_scale(dtype, n);
    KD_NOTE_PLUMBING(loss_kernel_name(sel.kernel));
    auto run = [&](auto z) {
        using T = decltype(z);
        hipLaunchKernelGGL(scale_by_device_scalar_kernel<T>, dim3(sel.blocks), dim3(256), 0, (hipStream_t)stream, (T *)x, (long long)(n / 8), (long long)n, scale);
    };
    switch (sel.kernel) {
    case LK_SCALE_F32: run(float{}); break;
    case LK_SCALE_BF16: run(bf16_t{}); break;
    default: return no_launch("kd_scale_by_device_scalar", sel);
    }
    KD_CHECK_LAUNCH("kd_scale_by_device_scalar");
    return KD_OK;
}

extern "C" int kd_radam_step_multi(const kd_radam_tensor *ts, int32_t count, kd_stream_t stream)
{
    KD_REQUIRE(ts && count > 0, KD_ERR_INVALID, "kd_radam_step_multi: bad argument");
    for (int i = 0; i < count; ++i)
        KD_REQUIRE(ts[i].p && ts[i].g && ts[i].exp_avg && ts[i].exp_avg_sq && ts[i].n > 0 && ts[i].step >= 1, KD_ERR_INVALID,
                   "kd_radam_step_multi: bad tensor %d", i);
    for (int done = 0; done < count;) {
        RadamBatch b;
        int nb = 0, k = 0;
        for (; k < RADAM_MAXT && done + k < count; ++k) {
            const kd_radam_tensor &t = ts[done + k];
            const long long blocks = (t.n + RADAM_BLK - 1) / RADAM_BLK;
            if (k > 0 && nb + blocks > 0x3fffffffLL) break;
            KD_REQUIRE(blocks <= 0x3fffffffLL, KD_ERR_UNSUPPORTED, "kd_radam_step_multi: tensor too large");
            int rect;
            double step_size;
            radam_constants(t.step, t.beta1, t.beta2, &rect, &step_size);
            b.p[k] = t.p; b.g[k] = t.g; b.m[k] = t.exp_avg; b.v[k] = t.exp_avg_sq; b.n[k] = t.n;
            b.blk0[k] = nb;
            b.wd_lr[k] = (float)((double)t.weight_decay * t.lr);
            b.step_lr[k] = (float)(step_size * t.lr);
            b.beta1[k] = t.beta1; b.beta2[k] = t.beta2; b.eps[k] = t.eps; b.rect[k] = rect;
            nb += (int)blocks;
        }
        b.blk0[k] = nb;
        b.count = k;
        KD_NOTE_PLUMBING(loss_kernel_name(LK_RADAM_MULTI));
        hipLaunchKernelGGL(radam_multi_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, b);
        KD_CHECK_LAUNCH("kd_radam_step_multi");
        done += k;
    }
    return KD_OK;
}
