// HBM-bound trunk plumbing around the convolutions: stem conv, max-pool (+BN/ReLU),
// bilinear align_corners upsample, ASPP image pooling, BN folding, strided copy/cast.
// Also hosts the error plumbing of the C-ABI.
#include <stdarg.h>
#include <pthread.h>
#include <string.h>

#include "kd_common.h"
#include "plumb_select.h"

static thread_local char g_err[512] = "";

void kd_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" int kd_version(void) { return 100; }
extern "C" const char *kd_last_error(void) { return g_err; }

// ---- kernel-selection log ---------------------------------------------------------------------------------------
// Host-side counters of which device kernel each dispatcher launched (tests assert that a shape reaches the kernel it is
// meant to cover; bench.py attributes event time to kernel classes).  Off by default: one relaxed load per launch.
namespace {
struct KernelLogEntry { const char *name; long long count; };
constexpr int KLOG_MAX = 128;
KernelLogEntry g_klog[KLOG_MAX];
int g_klog_n = 0;
volatile int g_klog_on = 0;
pthread_mutex_t g_klog_mu = PTHREAD_MUTEX_INITIALIZER;
thread_local const char *g_klog_last = "";
thread_local const char *g_plumbing_last = "";
}  // namespace

void kd_note_plumbing(const char *name) { g_plumbing_last = name; }

void kd_note_kernel(const char *name)
{
    g_klog_last = name;
    if (!g_klog_on) return;
    pthread_mutex_lock(&g_klog_mu);
    int i = 0;
    for (; i < g_klog_n; ++i)
        if (g_klog[i].name == name || !strcmp(g_klog[i].name, name)) break;
    if (i == g_klog_n && g_klog_n < KLOG_MAX) g_klog[g_klog_n++] = KernelLogEntry{name, 0};
    if (i < g_klog_n) ++g_klog[i].count;
    pthread_mutex_unlock(&g_klog_mu);
}

extern "C" int kd_debug_kernel_log_enable(int32_t on)
{
    pthread_mutex_lock(&g_klog_mu);
    g_klog_on = on ? 1 : 0;
    if (on) g_klog_n = 0;   // enabling starts a fresh log
    pthread_mutex_unlock(&g_klog_mu);
    return KD_OK;
}

extern "C" const char *kd_debug_last_kernel(void) { return g_klog_last; }
extern "C" const char *kd_debug_last_plumbing_kernel(void) { return g_plumbing_last; }

extern "C" int64_t kd_debug_kernel_log_read(char *buf, size_t bytes)
{
    // "name\tcount\n" per kernel seen since the log was enabled; returns the bytes needed (excluding the terminator)
    pthread_mutex_lock(&g_klog_mu);
    size_t need = 0;
    for (int i = 0; i < g_klog_n; ++i) {
        char line[256];
        const int n = snprintf(line, sizeof(line), "%s\t%lld\n", g_klog[i].name, g_klog[i].count);
        if (buf && need + (size_t)n < bytes) memcpy(buf + need, line, (size_t)n);
        need += (size_t)n;
    }
    if (buf && bytes) buf[need < bytes ? need : bytes - 1] = 0;
    pthread_mutex_unlock(&g_klog_mu);
    return (int64_t)need;
}

namespace {

// ---- stem conv 3 -> 64, 3x3, pad 1, NCHW fp32 in, NHWC out ---------------------------
// block = 64 pixels x 4 channel groups of 16; weights (27 x 64) in LDS.
template <typename T>
__global__ __launch_bounds__(256) void stem_conv_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                        T *__restrict__ y, int N, int H, int W)
{
    __shared__ __attribute__((aligned(16))) float wl[27 * 64];  // [ci*9 + ky*3 + kx][co]
    const int tid = threadIdx.x;
    for (int i = tid; i < 27 * 64; i += 256) {
        const int t = i >> 6, co = i & 63;
        wl[i] = w[co * 27 + t];
    }
    __syncthreads();
    const int cg = tid >> 6;  // 16-channel group (wave-uniform)
    const long long pix = (long long)blockIdx.x * 64 + (tid & 63);
    const long long HW = (long long)H * W;
    if (pix >= (long long)N * HW) return;
    const int n = (int)(pix / HW);
    const int rem = (int)(pix - (long long)n * HW);
    const int h = rem / W, ww = rem - h * W;
    float acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int hi = h - 1 + ky;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int wi = ww - 1 + kx;
                const bool ok = hi >= 0 && hi < H && wi >= 0 && wi < W;
                const int hc = hi < 0 ? 0 : (hi >= H ? H - 1 : hi), wc = wi < 0 ? 0 : (wi >= W ? W - 1 : wi);
                float v = x[((size_t)(n * 3 + ci) * H + hc) * W + wc];  // unconditional load, select after (no branch per tap)
                v = ok ? v : 0.f;
                const float *wr = &wl[(ci * 9 + ky * 3 + kx) * 64 + cg * 16];
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[q] = fmaf(v, wr[q], acc[q]);
            }
        }
    T *o = y + (size_t)pix * 64 + cg * 16;
    float lo[8], hi8[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { lo[q] = acc[q]; hi8[q] = acc[8 + q]; }
    st8(o, lo);
    st8(o + 8, hi8);
}

// bf16 variant on the matrix cores: K = 27 taps x channels (padded to 32), one v_mfma_f32_16x16x32_bf16 per 16 pixels x 16
// output channels.  A wave walks 16-pixel row segments: lane (pixel i, k-group q) gathers its 8 taps from the NCHW fp32
// image (16 consecutive pixels per tap: 64-B runs), the four weight fragments stay in registers, and the 16 x 64 result
// goes through a 2-KiB LDS patch so that every pixel's 128 B of channels leave as whole 32-B vectors.
typedef __attribute__((ext_vector_type(8))) short stem_bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float stem_f32x4_t;
__global__ __launch_bounds__(256) void stem_conv_mfma_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                             bf16_t *__restrict__ y, int N, int H, int W, int groups_per_row)
{
    constexpr int PSTR = 64 * 2 + 16;   // patch row stride (bytes): 16 pixels x 64 channels bf16, padded
    __shared__ __attribute__((aligned(16))) char patch[4][16 * PSTR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 15, kg = lane >> 4;
    // this lane's 8 taps: k = kg*8 + q = ci*9 + ky*3 + kx (k >= 27: zero)
    int toff[8], tdy[8], tdx[8];
    uint32_t tvalid = 0;
    const size_t HW = (size_t)H * W;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k = kg * 8 + q, kc = k < 27 ? k : 0;
        const int ci = kc / 9, ky = (kc % 9) / 3, kx = kc % 3;
        tdy[q] = ky - 1; tdx[q] = kx - 1;
        toff[q] = ci;
        tvalid |= k < 27 ? (1u << q) : 0u;
    }
    // weight fragments: lane (channel j = fi of tile t, k-group kg)
    uint4 bw[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int k = kg * 8 + q;
            v[q] = k < 27 ? w[(t * 16 + fi) * 27 + k] : 0.f;
        }
        bw[t] = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
    }
    char *pw = patch[wave];
    const long long ngroups = (long long)N * H * groups_per_row;
    for (long long g = (long long)blockIdx.x * 4 + wave; g < ngroups; g += (long long)gridDim.x * 4) {
        const int gx = (int)(g % groups_per_row);
        const long long rowid = g / groups_per_row;
        const int h = (int)(rowid % H), n = (int)(rowid / H);
        const int px = gx * 16 + fi;   // this lane's pixel column (may run past W in the last group)
        const float *xn = x + (size_t)n * 3 * HW;
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int hi = h + tdy[q], wi = px + tdx[q];
            const bool ok = ((tvalid >> q) & 1u) && hi >= 0 && hi < H && wi >= 0 && wi < W;
            const int hc = min(max(hi, 0), H - 1), wc = min(max(wi, 0), W - 1);
            const float t = xn[(size_t)toff[q] * HW + (size_t)hc * W + wc];   // unconditional load, select after
            v[q] = ok ? t : 0.f;
        }
        const uint4 a = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            stem_f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(stem_bf16x8_t, a), __builtin_bit_cast(stem_bf16x8_t, bw[t]),
                                                          acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) *(bf16_t *)(pw + (kg * 4 + r) * PSTR + (t * 16 + fi) * 2) = f32_to_bf16(acc[r]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        {
            const int p = lane >> 2, c = lane & 3;   // pixel of the group, 16-channel quarter
            const uint4 lo = *(const uint4 *)(pw + p * PSTR + c * 32), hi = *(const uint4 *)(pw + p * PSTR + c * 32 + 16);
            const int col = gx * 16 + p;
            if (col < W) {
                bf16_t *o = y + (((size_t)n * H + h) * W + col) * 64 + c * 16;
                *(uint4 *)o = lo;
                *(uint4 *)(o + 8) = hi;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// ---- stem conv + pool2 in one pass (frozen stem, bf16) ------------------------------------------------------------------
// mod1's 64-channel full-resolution output has one reader in DeepWV3Plus -- pool2 (wider_resnet.py: mod1 -> pool2 -> mod2) --
// so when nothing else needs it (frozen stem, no shape stream) it never has to reach HBM: 1.07 GB written and read back per
// network and step at 4 x 1024 x 2048.  A wave owns 7 pooled columns (16 stem columns 2*w0-1 .. 2*w0+14) and walks down a
// segment of pooled rows: per row it computes the two new stem rows on the matrix cores (same K = 27 -> 32 MFMA as above,
// operands swapped so a lane holds 4 consecutive channels of one pixel), keeps the previous odd row as the carry, takes the
// vertical maximum in fp32 registers, rounds it to bf16 into a 16-pixel LDS patch and finishes the horizontal maximum + the
// consumer's BN/ReLU when the patch is read back as 16-B channel vectors.  Rounding is monotone, so round(max) == max(round):
// the result is bit for bit what stem_conv_mfma_kernel + maxpool_kernel produce.
constexpr int SP_COLS = PLUMB_SP_COLS;      // pooled columns per wave
constexpr int SP_ROWS = PLUMB_SP_ROWS;      // pooled rows per wave segment
__global__ __launch_bounds__(256) void stem_pool_kernel(const float *__restrict__ x, const float *__restrict__ w, bf16_t *__restrict__ y_raw,
                                                        bf16_t *__restrict__ y_act, const float *__restrict__ scale,
                                                        const float *__restrict__ shift, int N, int H, int W, int Ho, int Wo,
                                                        int ngx, int nseg)
{
    constexpr int PSTR = 64 * 2 + 16;   // patch row stride (bytes): one pixel's 64 channels bf16, padded
    __shared__ __attribute__((aligned(16))) char patch[4][16 * PSTR];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fi = lane & 15, kg = lane >> 4;
    long long wid = (long long)blockIdx.x * 4 + wave;
    const long long nw = (long long)N * ngx * nseg;
    if (wid >= nw) return;   // wave-private work: no block-wide barrier below
    const int gx = (int)(wid % ngx); wid /= ngx;
    const int sg = (int)(wid % nseg);
    const int n = (int)(wid / nseg);
    const int w0 = gx * SP_COLS;
    const int col = 2 * w0 - 1 + fi;                 // this lane's stem column
    const bool col_ok = col >= 0 && col < W;
    // this lane's 8 taps: k = kg*8 + q = ci*9 + ky*3 + kx (k >= 27: zero)
    int tdy[8], tdx[8], tci[8];
    uint32_t tvalid = 0;
    const size_t HW = (size_t)H * W;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int k = kg * 8 + q, kc = k < 27 ? k : 0;
        tci[q] = kc / 9; tdy[q] = (kc % 9) / 3 - 1; tdx[q] = kc % 3 - 1;
        tvalid |= k < 27 ? (1u << q) : 0u;
    }
    // weight fragments as the A operand: lane (channel i = fi of tile t, k-group kg)
    uint4 bw[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int k = kg * 8 + q;
            v[q] = k < 27 ? w[(t * 16 + fi) * 27 + k] : 0.f;
        }
        bw[t] = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
    }
    const float *xn = x + (size_t)n * 3 * HW;
    const float NINF = -INFINITY;
    // one stem row for the 16 columns: D[channel][pixel], lane (pixel fi, kg) holds channels 16t + 4kg .. +3; rows / columns
    // outside the image are the pool's padding (-inf)
    auto stem_row = [&](int h, stem_f32x4_t (&o)[4]) __attribute__((always_inline)) {
        if (h < 0 || h >= H) {   // wave-uniform
#pragma unroll
            for (int t = 0; t < 4; ++t) o[t] = (stem_f32x4_t){NINF, NINF, NINF, NINF};
            return;
        }
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int hi = h + tdy[q], wi = col + tdx[q];
            const bool ok = ((tvalid >> q) & 1u) && hi >= 0 && hi < H && wi >= 0 && wi < W;
            const int hc = min(max(hi, 0), H - 1), wc = min(max(wi, 0), W - 1);
            const float tv = xn[(size_t)tci[q] * HW + (size_t)hc * W + wc];   // unconditional load, select after
            v[q] = ok ? tv : 0.f;
        }
        const uint4 a = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            stem_f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(stem_bf16x8_t, bw[t]), __builtin_bit_cast(stem_bf16x8_t, a),
                                                          acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) o[t][r] = col_ok ? acc[r] : NINF;
        }
    };
    // read-back role: lane = (pooled column m of the group, 8-channel vector c8)
    const int m = lane >> 3, c8 = lane & 7;
    float sc[8], sf[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        sc[q] = y_act ? scale[c8 * 8 + q] : 1.f;
        sf[q] = y_act ? shift[c8 * 8 + q] : 0.f;
    }
    char *pw = patch[wave];
    const int ho0 = sg * SP_ROWS, ho1 = min(ho0 + SP_ROWS, Ho);
    stem_f32x4_t carry[4], r0[4], r1[4];
    stem_row(2 * ho0 - 1, carry);
    for (int ho = ho0; ho < ho1; ++ho) {
        stem_row(2 * ho, r0);
        stem_row(2 * ho + 1, r1);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = fmaxf(fmaxf(carry[t][r], r0[t][r]), r1[t][r]);
                carry[t][r] = r1[t][r];
            }
            *(uint2 *)(pw + fi * PSTR + (t * 16 + kg * 4) * 2) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (m < SP_COLS && w0 + m < Wo) {
            float mx[8], t8[8];
            ld8((const bf16_t *)(pw + (2 * m) * PSTR + c8 * 16), mx);
            ld8((const bf16_t *)(pw + (2 * m + 1) * PSTR + c8 * 16), t8);
#pragma unroll
            for (int q = 0; q < 8; ++q) mx[q] = fmaxf(mx[q], t8[q]);
            ld8((const bf16_t *)(pw + (2 * m + 2) * PSTR + c8 * 16), t8);
#pragma unroll
            for (int q = 0; q < 8; ++q) mx[q] = fmaxf(mx[q], t8[q]);
            const size_t op = (((size_t)n * Ho + ho) * Wo + w0 + m) * 64 + c8 * 8;
            if (y_raw) st8(y_raw + op, mx);
            if (y_act) {
                float a8[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) a8[q] = fmaxf(fmaf(mx[q], sc[q], sf[q]), 0.f);
                st8(y_act + op, a8);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// ---- max-pool 3x3 / stride 2 / pad 1 (+ optional BN-eval + ReLU second output) ---------
template <typename T>
__global__ __launch_bounds__(256) void maxpool_kernel(const T *__restrict__ x, int ldx, T *__restrict__ y_raw, int ld_raw,
                                                      T *__restrict__ y_act, int ld_act, const float *__restrict__ scale,
                                                      const float *__restrict__ shift, int N, int H, int W, int C, int Ho,
                                                      int Wo)
{
    // grid: x = chunks of one output row's (Wo * C/8) vectors, y = output row, z = image
    const unsigned c8 = (unsigned)C >> 3;
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= (unsigned)Wo * c8) return;
    const unsigned wo = e / c8, cq = e - wo * c8;
    const int ho = blockIdx.y, n = blockIdx.z;
    {
        float m[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) m[q] = -INFINITY;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int hi = ho * 2 - 1 + ky;
            if (hi < 0 || hi >= H) continue;   // block-uniform
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int wi = (int)wo * 2 - 1 + kx;
                const int wc = wi < 0 ? 0 : (wi >= W ? W - 1 : wi);   // clamped tap duplicates a valid one: max unchanged
                float v[8];
                ld8(x + (((size_t)n * H + hi) * W + wc) * ldx + cq * 8, v);
#pragma unroll
                for (int q = 0; q < 8; ++q) m[q] = fmaxf(m[q], v[q]);
            }
        }
        const size_t op = ((size_t)n * Ho + ho) * Wo + wo;
        if (y_raw) st8(y_raw + op * ld_raw + cq * 8, m);
        if (y_act) {
            float a[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) a[q] = fmaxf(fmaf(m[q], scale[cq * 8 + q], shift[cq * 8 + q]), 0.f);
            st8(y_act + op * ld_act + cq * 8, a);
        }
    }
}

// ---- bilinear upsample, align_corners=True ---------------------------------------------
// grid: x = chunks of one output row's (Wo * C/VEC) elements, y = groups of UP_RO output rows, z = image.  A thread produces
// the UP_RO rows of its (column, channel vector): the column weights are computed once, and when enlarging, consecutive
// output rows interpolate between the same two input rows, whose four taps stay in registers (x8: 4 + 2 loads per 8 outputs
// instead of 32).  One thread per output element made 16 M short-lived threads with four dependent gathers each: 0.41 ms for
// a 1.07-GB output that a fill writes in 0.15 ms.  Rows are interpolated along x when loaded ((1-aw)*a + aw*b, as the reference
// does per output), then along y per output: the same expression tree, 2 instead of 7 operations per element.
constexpr int UP_RO = PLUMB_UP_RO;
template <typename TI, typename TO, int VEC>
__global__ __launch_bounds__(256) void upsample_kernel(const TI *__restrict__ x, int ldx, TO *__restrict__ y, int ldy, int N,
                                                       int H, int W, int C, int Ho, int Wo, float sh, float sw, float oh, float ow)
{
    const unsigned cv = (unsigned)C / VEC;
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= (unsigned)Wo * cv) return;
    const unsigned wo = e / cv, cq = e - wo * cv;
    const int n = blockIdx.z;
    int w0, w1; float aw;
    resample_src((int)wo, sw, ow, W, w0, w1, aw);
    const TI *b = x + (size_t)n * H * W * ldx + cq * VEC;
    float la[VEC], lb[VEC];                // the two cached input rows, already interpolated along x
    int ia = -1, ib = -1;                  // their row indices (block-uniform)
    auto load_row = [&](int h, float (&l)[VEC]) __attribute__((always_inline)) {
        float r0[VEC], r1[VEC];
        if constexpr (VEC == 8) {
            ld8(b + ((size_t)h * W + w0) * ldx, r0);
            ld8(b + ((size_t)h * W + w1) * ldx, r1);
        } else {
            r0[0] = Elem<TI>::ld(b + ((size_t)h * W + w0) * ldx);
            r1[0] = Elem<TI>::ld(b + ((size_t)h * W + w1) * ldx);
        }
#pragma unroll
        for (int q = 0; q < VEC; ++q) l[q] = resample_lerp(aw, r0[q], r1[q]);
    };
#pragma unroll
    for (int rr = 0; rr < UP_RO; ++rr) {
        const int ho = blockIdx.y * UP_RO + rr;
        if (ho >= Ho) break;
        int h0, h1; float ah;
        resample_src(ho, sh, oh, H, h0, h1, ah);
        if (h0 == ib && ia != h0) {        // slide: the lower row becomes the upper one
#pragma unroll
            for (int q = 0; q < VEC; ++q) la[q] = lb[q];
            ia = ib;
        }
        if (ia != h0) { load_row(h0, la); ia = h0; }
        if (ib != h1) {
            if (h1 == ia) {
#pragma unroll
                for (int q = 0; q < VEC; ++q) lb[q] = la[q];
            } else {
                load_row(h1, lb);
            }
            ib = h1;
        }
        const size_t o = (((size_t)n * Ho + ho) * Wo + wo) * ldy + cq * VEC;
        float v[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) v[q] = resample_lerp(ah, la[q], lb[q]);
        if constexpr (VEC == 8) st8(y + o, v);
        else Elem<TO>::st(y + o, v[0]);
    }
}

// Dense output rows whose channel count is not a multiple of 8 (the 19-class logits, fp32: 1.27 GB per 8 images): a thread owns
// FOUR consecutive floats of the flattened (wo, c) row -- up to two pixels -- and stores them as one 16-B vector; same expression
// tree per element, same row reuse over UP_RO output rows.  (Measured: 520 us against 532 us for the 4-B-store kernel above at
// 8 images -- the store width is not what holds this kernel at 2.4 TB/s; kept for the quarter of the store instructions.)
template <typename TI>
__global__ __launch_bounds__(256) void upsample_flat4_kernel(const TI *__restrict__ x, int ldx, float *__restrict__ y, int N, int H, int W,
                                                             int C, int Ho, int Wo, float sh, float sw, float oh, float ow)
{
    const unsigned e4 = blockIdx.x * 256u + threadIdx.x;
    if (e4 * 4u >= (unsigned)Wo * (unsigned)C) return;
    const int n = blockIdx.z;
    int w0[4], w1[4], cc[4];
    float aw[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned f = e4 * 4u + q, wo = f / (unsigned)C;
        cc[q] = (int)(f - wo * (unsigned)C);
        resample_src((int)wo, sw, ow, W, w0[q], w1[q], aw[q]);
    }
    const TI *b = x + (size_t)n * H * W * ldx;
    float la[4], lb[4];
    int ia = -1, ib = -1;
    auto load_row = [&](int h, float (&l)[4]) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float r0 = Elem<TI>::ld(b + ((size_t)h * W + w0[q]) * ldx + cc[q]);
            const float r1 = Elem<TI>::ld(b + ((size_t)h * W + w1[q]) * ldx + cc[q]);
            l[q] = resample_lerp(aw[q], r0, r1);
        }
    };
#pragma unroll
    for (int rr = 0; rr < UP_RO; ++rr) {
        const int ho = blockIdx.y * UP_RO + rr;
        if (ho >= Ho) break;
        int h0, h1; float ah;
        resample_src(ho, sh, oh, H, h0, h1, ah);
        if (h0 == ib && ia != h0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) la[q] = lb[q];
            ia = ib;
        }
        if (ia != h0) { load_row(h0, la); ia = h0; }
        if (ib != h1) {
            if (h1 == ia) {
#pragma unroll
                for (int q = 0; q < 4; ++q) lb[q] = la[q];
            } else {
                load_row(h1, lb);
            }
            ib = h1;
        }
        float4 v;
        v.x = resample_lerp(ah, la[0], lb[0]);
        v.y = resample_lerp(ah, la[1], lb[1]);
        v.z = resample_lerp(ah, la[2], lb[2]);
        v.w = resample_lerp(ah, la[3], lb[3]);
        *(float4 *)(y + (((size_t)n * Ho + ho) * Wo) * C + (size_t)e4 * 4) = v;
    }
}

// ---- ASPP image pooling ------------------------------------------------------------------
constexpr int GAP_CHUNKS = PLUMB_GAP_CHUNKS;
// partial[chunk][n][c] = sum over the chunk's pixels; block = 32 channel octets x 8 pixel lanes
template <typename T>
__global__ __launch_bounds__(256) void gap_partial_kernel(const T *__restrict__ x, int ldx, float *__restrict__ partial,
                                                          int N, int HW, int C)
{
    __shared__ float red[8][256 + 8];
    const int co = threadIdx.x & 31, pl = threadIdx.x >> 5;
    const int c = blockIdx.y * 256 + co * 8;
    const int n = blockIdx.z, chunk = blockIdx.x;
    const int per = (HW + GAP_CHUNKS - 1) / GAP_CHUNKS;
    const int p0 = chunk * per, p1 = min(HW, p0 + per);
    float s[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) s[q] = 0.f;
    if (c < C)
        for (int p = p0 + pl; p < p1; p += 8) {
            float v[8];
            ld8(x + ((size_t)n * HW + p) * ldx + c, v);
#pragma unroll
            for (int q = 0; q < 8; ++q) s[q] += v[q];
        }
#pragma unroll
    for (int q = 0; q < 8; ++q) red[pl][co * 8 + q] = s[q];
    __syncthreads();
    const int cc = threadIdx.x;
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += red[k][cc];
    if (blockIdx.y * 256 + cc < C) partial[((size_t)chunk * N + n) * C + blockIdx.y * 256 + cc] = t;
}
// mean[n][c], then out[n][co] = relu(scale*dot(w[co], mean[n]) + shift); one block per (co-block of 4 waves, n)
__global__ __launch_bounds__(256) void gap_finish_kernel(const float *__restrict__ partial, float *__restrict__ mean,
                                                         int N, int HW, int C)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * C) return;
    float s = 0.f;
    for (int k = 0; k < GAP_CHUNKS; ++k) s += partial[(size_t)k * N * C + i];
    mean[i] = s / (float)HW;
}
// mean[n][c] from the partial rows a conv epilogue wrote while it produced the pooled tensor (kd_conv_epilogue.bn_sums without a
// mask: part[row][0][c] = sum over 128 pixels): rows n * rpi .. + rpi - 1 belong to image n, added in row order (fixed: bit-reproducible)
__global__ __launch_bounds__(256) void gap_rows_finish_kernel(const float *__restrict__ part, float *__restrict__ mean, int N, int rpi,
                                                              int HW, int C)
{
    // block = 32 channels x 8 row slices of one image; a slice's rows are added in order, then the 8 slices in order
    __shared__ float red[8][32];
    const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl, n = blockIdx.y;
    const int per = (rpi + 7) / 8, r0 = sl * per, r1 = min(rpi, r0 + per);
    float s = 0.f;
    if (c < C) {
        const float *src = part + (size_t)n * rpi * 2 * C + c;
        for (int r = r0; r < r1; ++r) s += src[(size_t)r * 2 * C];
    }
    red[sl][cl] = s;
    __syncthreads();
    if (sl == 0 && c < C) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += red[k][cl];
        mean[(size_t)n * C + c] = t / (float)HW;
    }
}
__global__ __launch_bounds__(256) void img_conv_kernel(const float *__restrict__ mean, const float *__restrict__ w,
                                                       const float *__restrict__ scale, const float *__restrict__ shift,
                                                       float *__restrict__ out, int Cin, int Cout)
{
    // one wave per output channel
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int co = blockIdx.x * 4 + wv, n = blockIdx.y;
    if (co >= Cout) return;
    float s = 0.f;
    for (int ci = lane; ci < Cin; ci += 64) s = fmaf(w[(size_t)co * Cin + ci], mean[(size_t)n * Cin + ci], s);
    s = wave_sum(s);
    if (lane == 0) out[(size_t)n * Cout + co] = fmaxf(s * scale[co] + shift[co], 0.f);
}
template <typename T>
__global__ __launch_bounds__(256) void broadcast_kernel(const float *__restrict__ v, T *__restrict__ y, int ldy, int N,
                                                        int HW, int C)
{
    const int c8 = C >> 3;
    const long long total = (long long)N * HW * c8;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int cq = (int)(i % c8);
        const long long pix = i / c8;
        const int n = (int)(pix / HW);
        float t[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) t[q] = v[(size_t)n * C + cq * 8 + q];
        st8(y + (size_t)pix * ldy + cq * 8, t);
    }
}

__global__ void bn_fold_kernel(const float *g, const float *b, const float *m, const float *v, float eps, float *scale,
                               float *shift, int C)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float sc = g[c] / sqrtf(v[c] + eps);
    scale[c] = sc;
    shift[c] = b[c] - m[c] * sc;
}

__global__ __launch_bounds__(256) void copy_cast_kernel(const void *src, int sdt, long long s_sN, long long s_sC,
                                                        long long s_sP, void *dst, int ddt, long long d_sN, long long d_sC,
                                                        long long d_sP, int N, int C, long long P, int c_fast)
{
    const long long total = (long long)N * C * P;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long n, c, p;
        if (c_fast) { c = i % C; const long long r = i / C; p = r % P; n = r / P; }
        else { p = i % P; const long long r = i / P; c = r % C; n = r / C; }
        kd_st(dst, ddt, n * d_sN + c * d_sC + p * d_sP, kd_ld(src, sdt, n * s_sN + c * s_sC + p * s_sP));
    }
}

inline dim3 dim3_of(const PlumbGrid &g) { return dim3(g.x, g.y, g.z); }

}  // namespace

// Every entry point below: its argument checks, its selector (plumb_select.h), the selected kernel's name noted once, then a
// switch over sel.kernel to the instantiation on the selector's grid.
extern "C" int kd_stem_conv(int32_t dtype, const float *x_nchw, const float *w, void *y, int32_t N, int32_t H, int32_t W,
                            kd_stream_t stream)
{
    KD_REQUIRE(x_nchw && w && y && N > 0 && H > 0 && W > 0, KD_ERR_INVALID, "kd_stem_conv: bad argument");
    KD_REQUIRE(plumb_dtype_ok(dtype), KD_ERR_INVALID, "kd_stem_conv: bad dtype");
    KD_REQUIRE(kd_aligned16(y), KD_ERR_INVALID, "kd_stem_conv: y must be 16-B aligned");
    const PlumbSel sel = plumb_select_stem_conv(dtype, N, H, W);
    hipStream_t s = (hipStream_t)stream;
    KD_NOTE_PLUMBING(plumb_kernel_name(sel.kernel));
    if (sel.kernel == PK_STEM_CONV_MFMA) {
        KD_NOTE_KERNEL("stem_conv_mfma_kernel");
        hipLaunchKernelGGL(stem_conv_mfma_kernel, dim3_of(sel.grid), dim3(256), 0, s, x_nchw, w, (bf16_t *)y, N, H, W, sel.ngx);
    } else {
        KD_NOTE_KERNEL("stem_conv_kernel<f32>");
        hipLaunchKernelGGL(stem_conv_kernel<float>, dim3_of(sel.grid), dim3(256), 0, s, x_nchw, w, (float *)y, N, H, W);
    }
    KD_CHECK_LAUNCH("kd_stem_conv");
    return KD_OK;
}

extern "C" int kd_stem_conv_pool(const float *x_nchw, const float *w, void *y_raw, void *y_act, const float *scale,
                                 const float *shift, int32_t N, int32_t H, int32_t W, kd_stream_t stream)
{
    KD_REQUIRE(x_nchw && w && (y_raw || y_act) && N > 0 && H > 0 && W > 0, KD_ERR_INVALID, "kd_stem_conv_pool: bad argument");
    KD_REQUIRE(!y_act || (scale && shift), KD_ERR_INVALID, "kd_stem_conv_pool: y_act needs scale/shift");
    KD_REQUIRE((!y_raw || kd_aligned16(y_raw)) && (!y_act || kd_aligned16(y_act)), KD_ERR_INVALID,
               "kd_stem_conv_pool: outputs must be 16-B aligned");
    const PlumbSel sel = plumb_select_stem_conv_pool(N, H, W);
    KD_REQUIRE(sel.kernel != PLUMB_REFUSED, KD_ERR_UNSUPPORTED, "kd_stem_conv_pool: image too large");
    KD_NOTE_KERNEL("stem_pool_kernel");
    KD_NOTE_PLUMBING(plumb_kernel_name(sel.kernel));
    hipLaunchKernelGGL(stem_pool_kernel, dim3_of(sel.grid), dim3(256), 0, (hipStream_t)stream, x_nchw, w, (bf16_t *)y_raw,
                       (bf16_t *)y_act, scale, shift, N, H, W, sel.Ho, sel.Wo, sel.ngx, sel.nseg);
    KD_CHECK_LAUNCH("kd_stem_conv_pool");
    return KD_OK;
}

extern "C" int kd_maxpool3x3s2(int32_t dtype, const void *x, int32_t ldx, void *y_raw, int32_t ld_raw, void *y_act,
                               int32_t ld_act, const float *scale, const float *shift, int32_t N, int32_t H, int32_t W,
                               int32_t C, kd_stream_t stream)
{
    KD_REQUIRE(x && (y_raw || y_act), KD_ERR_INVALID, "kd_maxpool3x3s2: null argument");
    KD_REQUIRE(plumb_dtype_ok(dtype), KD_ERR_INVALID, "kd_maxpool3x3s2: bad dtype");
    KD_REQUIRE(!y_act || (scale && shift), KD_ERR_INVALID, "kd_maxpool3x3s2: y_act needs scale/shift");
    const int es = kd_elem_size(dtype);
    KD_REQUIRE(C % 8 == 0 && plumb_vec_ok(x, ldx, es) && plumb_vec_ok(y_raw, ld_raw, es) && plumb_vec_ok(y_act, ld_act, es), KD_ERR_INVALID,
               "kd_maxpool3x3s2: C %% 8 and 16-B alignment required");
    const PlumbSel sel = plumb_select_maxpool(dtype, N, H, W, C);
    const dim3 g = dim3_of(sel.grid);
    hipStream_t s = (hipStream_t)stream;
    KD_NOTE_PLUMBING(plumb_kernel_name(sel.kernel));
    if (sel.kernel == PK_MAXPOOL_BF16)
        hipLaunchKernelGGL(maxpool_kernel<bf16_t>, g, dim3(256), 0, s, (const bf16_t *)x, ldx, (bf16_t *)y_raw, ld_raw,
                           (bf16_t *)y_act, ld_act, scale, shift, N, H, W, C, sel.Ho, sel.Wo);
    else
        hipLaunchKernelGGL(maxpool_kernel<float>, g, dim3(256), 0, s, (const float *)x, ldx, (float *)y_raw, ld_raw,
                           (float *)y_act, ld_act, scale, shift, N, H, W, C, sel.Ho, sel.Wo);
    KD_CHECK_LAUNCH("kd_maxpool3x3s2");
    return KD_OK;
}

extern "C" int kd_upsample_bilinear(const void *x, int32_t x_dtype, int32_t ldx, void *y, int32_t y_dtype, int32_t ldy, int32_t N,
                                    int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, int32_t align_corners, kd_stream_t stream)
{
    KD_REQUIRE(x && y && N > 0 && H > 0 && W > 0 && C > 0 && Ho > 0 && Wo > 0, KD_ERR_INVALID,
               "kd_upsample_bilinear_ac: bad argument");
    KD_REQUIRE(plumb_dtype_ok(x_dtype) && plumb_dtype_ok(y_dtype), KD_ERR_INVALID, "kd_upsample_bilinear_ac: bad dtype");
    const PlumbSel sel = plumb_select_upsample(x, x_dtype, ldx, y, y_dtype, ldy, N, H, W, C, Ho, Wo, align_corners);
    const dim3 g = dim3_of(sel.grid);
    hipStream_t s = (hipStream_t)stream;
    KD_NOTE_PLUMBING(plumb_kernel_name(sel.kernel));
#define KD_UP(TI, TO, VEC)                                                                                                              \
    hipLaunchKernelGGL((upsample_kernel<TI, TO, VEC>), g, dim3(256), 0, s, (const TI *)x, ldx, (TO *)y, ldy, N, H, W, C, Ho, Wo, sel.sh, \
                       sel.sw, sel.oh, sel.ow);                                                                                         \
    break
#define KD_UP_FLAT4(TI)                                                                                                                  \
    hipLaunchKernelGGL((upsample_flat4_kernel<TI>), g, dim3(256), 0, s, (const TI *)x, ldx, (float *)y, N, H, W, C, Ho, Wo, sel.sh, sel.sw, \
                       sel.oh, sel.ow);                                                                                                  \
    break
    switch (sel.kernel) {
    case PK_UP_FLAT4_BF16: KD_UP_FLAT4(bf16_t);
    case PK_UP_BF16_BF16_8: KD_UP(bf16_t, bf16_t, 8);
    case PK_UP_BF16_BF16_1: KD_UP(bf16_t, bf16_t, 1);
    case PK_UP_BF16_F32_8: KD_UP(bf16_t, float, 8);
    case PK_UP_BF16_F32_1: KD_UP(bf16_t, float, 1);
    case PK_UP_FLAT4_F32: KD_UP_FLAT4(float);
    case PK_UP_F32_BF16_8: KD_UP(float, bf16_t, 8);
    case PK_UP_F32_BF16_1: KD_UP(float, bf16_t, 1);
    case PK_UP_F32_F32_8: KD_UP(float, float, 8);
    default: KD_UP(float, float, 1);
    }
#undef KD_UP
#undef KD_UP_FLAT4
    KD_CHECK_LAUNCH("kd_upsample_bilinear_ac");
    return KD_OK;
}

extern "C" int kd_upsample_bilinear_ac(const void *x, int32_t x_dtype, int32_t ldx, void *y, int32_t y_dtype, int32_t ldy,
                                       int32_t N, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo,
                                       kd_stream_t stream)
{
    return kd_upsample_bilinear(x, x_dtype, ldx, y, y_dtype, ldy, N, H, W, C, Ho, Wo, 1, stream);
}

extern "C" size_t kd_aspp_image_pool_workspace(int32_t N, int32_t Cin, int32_t Cout) { return plumb_image_pool_workspace(N, Cin, Cout); }

// the last two launches of both image-pooling entry points: mean[n][ci] -> pooled vector [n][co] -> every pixel of y (defined
// below them, so that the code object goes on listing the pooling kernels in front of the broadcast)
static int image_pool_tail(const PlumbSel &sel, const char *who, const float *mean, float *vec, const float *w, const float *scale,
                           const float *shift, void *y, int ldy, int N, int HW, int Cin, int Cout, hipStream_t s);

extern "C" int kd_aspp_image_pool(int32_t dtype, const void *x, int32_t ldx, const float *w, const float *scale,
                                  const float *shift, void *y, int32_t ldy, int32_t N, int32_t H, int32_t W, int32_t Cin,
                                  int32_t Cout, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    KD_REQUIRE(x && w && scale && shift && y && workspace, KD_ERR_INVALID, "kd_aspp_image_pool: null argument");
    KD_REQUIRE(plumb_dtype_ok(dtype), KD_ERR_INVALID, "kd_aspp_image_pool: bad dtype");
    const int es = kd_elem_size(dtype);
    KD_REQUIRE(Cin % 8 == 0 && Cout % 8 == 0 && kd_aligned16(x) && kd_aligned16(y) && (ldx * es) % 16 == 0 && (ldy * es) % 16 == 0,
               KD_ERR_INVALID, "kd_aspp_image_pool: channels %% 8 and 16-B alignment required");
    KD_REQUIRE(workspace_bytes >= plumb_image_pool_workspace(N, Cin, Cout), KD_ERR_WORKSPACE, "kd_aspp_image_pool: workspace too small");
    const PlumbSel sel = plumb_select_image_pool(dtype, N, H, W, Cin, Cout);
    float *partial = (float *)((char *)workspace + sel.ws_off[0]), *mean = (float *)((char *)workspace + sel.ws_off[1]);
    float *vec = (float *)((char *)workspace + sel.ws_off[2]);
    const int HW = H * W;
    hipStream_t s = (hipStream_t)stream;
    KD_NOTE_PLUMBING(plumb_kernel_name(sel.kernel));
    if (sel.kernel == PK_GAP_PARTIAL_BF16) hipLaunchKernelGGL(gap_partial_kernel<bf16_t>, dim3_of(sel.grid), dim3(256), 0, s, (const bf16_t *)x, ldx, partial, N, HW, Cin);
    else hipLaunchKernelGGL(gap_partial_kernel<float>, dim3_of(sel.grid), dim3(256), 0, s, (const float *)x, ldx, partial, N, HW, Cin);
    KD_CHECK_LAUNCH("kd_aspp_image_pool(partial)");
    hipLaunchKernelGGL(gap_finish_kernel, dim3((N * Cin + 255) / 256), dim3(256), 0, s, partial, mean, N, HW, Cin);   // a thread per (n, ci)
    KD_CHECK_LAUNCH("kd_aspp_image_pool");
    return image_pool_tail(sel, "kd_aspp_image_pool", mean, vec, w, scale, shift, y, ldy, N, HW, Cin, Cout, s);
}

/* kd_aspp_image_pool with the pooled sums already taken: part = the [N*H*W/128][2][Cin] partial rows kd_conv2d_fwd /
 * kd_conv1x1_dual_fwd wrote into ep->bn_sums (no mask) while producing the tensor.  H*W % 128 == 0 (an image is whole rows).
 * workspace: kd_aspp_image_pool_workspace(N, Cin, Cout). */
extern "C" int kd_aspp_image_pool_sums(int32_t dtype, const float *part, const float *w, const float *scale, const float *shift, void *y,
                                       int32_t ldy, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, void *workspace,
                                       size_t workspace_bytes, kd_stream_t stream)
{
    KD_REQUIRE(part && w && scale && shift && y && workspace, KD_ERR_INVALID, "kd_aspp_image_pool_sums: null argument");
    KD_REQUIRE(plumb_dtype_ok(dtype), KD_ERR_INVALID, "kd_aspp_image_pool_sums: bad dtype");
    const int es = kd_elem_size(dtype);
    KD_REQUIRE(Cout % 8 == 0 && kd_aligned16(y) && (ldy * es) % 16 == 0, KD_ERR_INVALID, "kd_aspp_image_pool_sums: Cout %% 8 and 16-B alignment required");
    KD_REQUIRE(N > 0 && H > 0 && W > 0 && (H * W) % 128 == 0, KD_ERR_INVALID, "kd_aspp_image_pool_sums: an image must be a whole number of 128-pixel rows");
    KD_REQUIRE(workspace_bytes >= plumb_image_pool_workspace(N, Cin, Cout), KD_ERR_WORKSPACE, "kd_aspp_image_pool_sums: workspace too small");
    const PlumbSel sel = plumb_select_image_pool_sums(dtype, N, H, W, Cin, Cout);
    float *mean = (float *)((char *)workspace + sel.ws_off[1]), *vec = (float *)((char *)workspace + sel.ws_off[2]);
    const int HW = H * W;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(gap_rows_finish_kernel, dim3_of(sel.grid), dim3(256), 0, s, part, mean, N, HW / 128, HW, Cin);
    KD_CHECK_LAUNCH("kd_aspp_image_pool_sums");
    return image_pool_tail(sel, "kd_aspp_image_pool_sums", mean, vec, w, scale, shift, y, ldy, N, HW, Cin, Cout, s);
}

static int image_pool_tail(const PlumbSel &sel, const char *who, const float *mean, float *vec, const float *w, const float *scale,
                           const float *shift, void *y, int ldy, int N, int HW, int Cin, int Cout, hipStream_t s)
{
    hipLaunchKernelGGL(img_conv_kernel, dim3((Cout + 3) / 4, N), dim3(256), 0, s, mean, w, scale, shift, vec, Cin, Cout);   // a wave per output channel
    KD_CHECK_LAUNCH(who);
    if (sel.kernel == PK_GAP_PARTIAL_BF16) hipLaunchKernelGGL(broadcast_kernel<bf16_t>, dim3_of(sel.grid2), dim3(256), 0, s, vec, (bf16_t *)y, ldy, N, HW, Cout);
    else hipLaunchKernelGGL(broadcast_kernel<float>, dim3_of(sel.grid2), dim3(256), 0, s, vec, (float *)y, ldy, N, HW, Cout);
    KD_CHECK_LAUNCH(who);
    return KD_OK;
}

extern "C" int kd_bn_fold(const float *gamma, const float *beta, const float *mean, const float *var, float eps,
                          float *scale, float *shift, int32_t C, kd_stream_t stream)
{
    KD_REQUIRE(gamma && beta && mean && var && scale && shift && C > 0, KD_ERR_INVALID, "kd_bn_fold: bad argument");
    const PlumbSel sel = plumb_select_bn_fold(C);
    KD_NOTE_PLUMBING(plumb_kernel_name(sel.kernel));
    hipLaunchKernelGGL(bn_fold_kernel, dim3_of(sel.grid), dim3(256), 0, (hipStream_t)stream, gamma, beta, mean, var, eps, scale, shift, C);
    KD_CHECK_LAUNCH("kd_bn_fold");
    return KD_OK;
}

extern "C" int kd_copy_cast(const void *src, int32_t src_dtype, int64_t s_sN, int64_t s_sC, int64_t s_sP, void *dst,
                            int32_t dst_dtype, int64_t d_sN, int64_t d_sC, int64_t d_sP, int32_t N, int32_t C, int64_t P,
                            kd_stream_t stream)
{
    KD_REQUIRE(src && dst && N > 0 && C > 0 && P > 0, KD_ERR_INVALID, "kd_copy_cast: bad argument");
    KD_REQUIRE(plumb_dtype_ok(src_dtype) && plumb_dtype_ok(dst_dtype), KD_ERR_INVALID, "kd_copy_cast: bad dtype");
    const PlumbSel sel = plumb_select_copy_cast(d_sC, N, C, P);
    KD_NOTE_PLUMBING(plumb_kernel_name(sel.kernel));
    hipLaunchKernelGGL(copy_cast_kernel, dim3_of(sel.grid), dim3(256), 0, (hipStream_t)stream, src, src_dtype, (long long)s_sN,
                       (long long)s_sC, (long long)s_sP, dst, dst_dtype, (long long)d_sN, (long long)d_sC, (long long)d_sP, N, C,
                       (long long)P, sel.kernel == PK_COPY_CAST_CFAST ? 1 : 0);
    KD_CHECK_LAUNCH("kd_copy_cast");
    return KD_OK;
}
