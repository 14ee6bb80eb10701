// One training batch of Cityscapes from the device-resident dataset in three stages (include/kdcc.h: kd_seg_crop, kd_seg_jitter,
// kd_seg_finish), a restatement of the reference's per-image chain (data_loader/joint_transforms.py:346-373, 75-123,
// data_loader/transforms.py:238-304, 101-110) whose random draws and whose double-precision tables arrive in a per-sample row
// (data_loader/seg_tables.py documents the words):
//   crop    PIL's bicubic resize restricted to the crop: the horizontal pass over the source rows a tile needs, rounded and clipped
//           to bytes in LDS, then the vertical pass, both in PIL's 22-bit integer arithmetic from host tables; the mask by nearest
//           source indices; the reference's pad (image 0, mask 255); the flip as a mirrored store.
//   jitter  brightness, contrast, saturation and hue as byte -> byte functions of a pixel in the row's order; the grey mean contrast
//           blends against is an exact integer sum: one pointwise pass up to contrast that also reduces, one from contrast on.
//   finish  scipy's symmetric Gaussian along rows then columns of byte / 255. in double (fixed order, no contraction), * 255 and
//           truncated; or the bytes as they are; then the 3 x 256 normalisation table, the output's dtype and layout, the int64 mask.
// Integer stages are exact; the float stages use IEEE operations in one order with contraction off, so the host-tensor path of the
// loader produces the same bits with torch ops.  Which instantiation runs is seg_data_select.h's decision; the launchers only launch.
// Every index a kernel forms from the table is re-checked against the source's extent: a bad row reads padding, never out of bounds.
#include <limits.h>

#include "kd_common.h"
#include "seg_data_select.h"

#pragma clang fp contract(off)

namespace {

constexpr int TPB = SEG_TPB, TX = SEG_TX, TY = SEG_TY, HDR = SEG_HDR, TAPS = SEG_TAPS, ENTRY = SEG_ENTRY, CAP_C = SEG_CAP_C, CAP_R = SEG_CAP_R;
constexpr int SRC_WORDS = (CAP_C * 3 + 6) / 4 + 1;     // 4-byte words of one staged source row, its start rounded down to a word
constexpr int PRECISION_BITS = 22;
constexpr int RMAX = SEG_MAX_RADIUS;
enum { I_INDEX = 0, I_FLIP = 7, I_ORDER = 8, I_FB = 12, I_FC = 13, I_FS = 14, I_HUE = 15, I_RADIUS = 16, I_JITTER = 17, I_WEIGHTS = 20 };
enum { OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3 };

__device__ __forceinline__ long long sample_index(const int32_t *row, long long n)
{
    const long long idx = row[I_INDEX];
    return idx < 0 ? 0 : (idx >= n ? n - 1 : idx);
}
__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// an entry [xmin, taps, k...] is a window inside [0, extent); anything else is padding
__device__ __forceinline__ bool entry_ok(const int32_t *e, int extent)
{
    return e[0] >= 0 && e[1] >= 1 && e[1] <= TAPS && e[0] <= extent - e[1];
}

// ---------------------------------------------------------------------------------------------------- resample + pad + crop + flip
// One workgroup per TY x TX tile of one sample's crop, in the crop's coordinates BEFORE the flip.  G: bytes per store.
template <int G>
__global__ __launch_bounds__(TPB) void seg_crop_kernel(const uint8_t *__restrict__ data, const uint8_t *__restrict__ targets, long long n, int H, int W,
                                                       const int32_t *__restrict__ params, long long pld, int S, uint8_t *__restrict__ img_out,
                                                       uint8_t *__restrict__ mask_out)
{
    __shared__ uint32_t sSrc[CAP_R * SRC_WORDS];
    __shared__ uint8_t sT[CAP_R * TX * 3];
    __shared__ alignas(16) uint8_t sImg[TY * TX * 3];
    __shared__ alignas(16) uint8_t sMsk[TY * TX];
    __shared__ int32_t sH[TX * ENTRY], sV[TY * ENTRY];
    __shared__ int sBound[4];
    const int tid = threadIdx.x, b = blockIdx.z, x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    const int nx = min(TX, S - x0), ny = min(TY, S - y0);
    const int32_t *row = params + b * pld;
    const int32_t *ht = row + HDR, *vt = ht + (long long)ENTRY * S, *mxs = vt + (long long)ENTRY * S, *mys = mxs + S;
    const long long idx = sample_index(row, n);
    const bool flip = row[I_FLIP] != 0;
    const long long total = n * H * W * 3;

    if (tid < 4) sBound[tid] = (tid & 1) ? 0 : INT_MAX;
    for (int i = tid; i < nx * ENTRY; i += TPB) sH[i] = ht[(long long)x0 * ENTRY + i];
    for (int i = tid; i < ny * ENTRY; i += TPB) sV[i] = vt[(long long)y0 * ENTRY + i];
    __syncthreads();
    if (tid < nx) {
        const int32_t *e = sH + tid * ENTRY;
        if (entry_ok(e, W)) atomicMin(&sBound[0], e[0]), atomicMax(&sBound[1], e[0] + e[1]);
    } else if (tid >= 64 && tid < 64 + ny) {
        const int32_t *e = sV + (tid - 64) * ENTRY;
        if (entry_ok(e, H)) atomicMin(&sBound[2], e[0]), atomicMax(&sBound[3], e[0] + e[1]);
    }
    __syncthreads();
    const int lo_c = sBound[0], hi_c = sBound[1], lo_r = sBound[2], hi_r = sBound[3];
    const int cols = hi_c - lo_c, rows = hi_r - lo_r;
    const bool any = cols >= 1 && rows >= 1 && cols <= CAP_C && rows <= CAP_R;      // else: the tile is padding throughout
    if (any) {
        // the source window, rows of 4-byte words from each row's start rounded down to a word
        const int wpr = (cols * 3 + 6) / 4;
        for (int i = tid; i < rows * wpr; i += TPB) {
            const int r = i / wpr, k = i - r * wpr;
            const long long a = ((idx * H + lo_r + r) * W + lo_c) * 3, a0 = (a & ~3LL) + 4 * k;
            uint32_t v = 0;
            if (a0 + 4 <= total) v = *(const uint32_t *)(data + a0);
            else
                for (int j = 0; j < 4; ++j)
                    if (a0 + j < total) v |= (uint32_t)data[a0 + j] << (8 * j);
            sSrc[r * SRC_WORDS + k] = v;
        }
        __syncthreads();
        const uint8_t *src = (const uint8_t *)sSrc;
        for (int i = tid; i < rows * nx * 3; i += TPB) {
            const int c = i % 3, xc = i / 3 % nx, r = i / (3 * nx);
            const int32_t *e = sH + xc * ENTRY;
            int out = 0;
            if (entry_ok(e, W)) {
                const int sh = (int)((((idx * H + lo_r + r) * W + lo_c) * 3) & 3);
                const uint8_t *p = src + r * SRC_WORDS * 4 + sh + (e[0] - lo_c) * 3 + c;
                int acc = 1 << (PRECISION_BITS - 1);
                for (int t = 0; t < e[1]; ++t) acc += e[2 + t] * (int)p[3 * t];
                out = clip8(acc >> PRECISION_BITS);
            }
            sT[(r * TX + xc) * 3 + c] = (uint8_t)out;
        }
        __syncthreads();
    }
    for (int i = tid; i < ny * nx * 3; i += TPB) {
        const int c = i % 3, xc = i / 3 % nx, y = i / (3 * nx);
        const int32_t *ex = sH + xc * ENTRY, *ey = sV + y * ENTRY;
        int out = 0;
        if (any && entry_ok(ex, W) && entry_ok(ey, H)) {
            const uint8_t *p = sT + ((ey[0] - lo_r) * TX + xc) * 3 + c;
            int acc = 1 << (PRECISION_BITS - 1);
            for (int t = 0; t < ey[1]; ++t) acc += ey[2 + t] * (int)p[3 * TX * t];
            out = clip8(acc >> PRECISION_BITS);
        }
        sImg[(y * TX + (flip ? nx - 1 - xc : xc)) * 3 + c] = (uint8_t)out;
    }
    for (int i = tid; i < ny * nx; i += TPB) {
        const int xc = i % nx, y = i / nx;
        const int sx = mxs[x0 + xc], sy = mys[y0 + y];
        int m = 255;
        if (sx >= 0 && sx < W && sy >= 0 && sy < H && entry_ok(sH + xc * ENTRY, W) && entry_ok(sV + y * ENTRY, H))
            m = targets[(idx * H + sy) * W + sx];
        sMsk[y * TX + (flip ? nx - 1 - xc : xc)] = (uint8_t)m;
    }
    __syncthreads();
    const int X0 = flip ? S - x0 - nx : x0;
    if constexpr (G == 16) {        // S % 16 == 0: nx is 16 or 32 and X0 a multiple of 16
        const int ppr = nx * 3 / 16, mpr = nx / 16;
        for (int i = tid; i < ny * ppr; i += TPB) {
            const int y = i / ppr, k = i - y * ppr;
            *(uint4 *)(img_out + (((long long)b * S + y0 + y) * S + X0) * 3 + 16 * k) = *(const uint4 *)(sImg + y * TX * 3 + 16 * k);
        }
        for (int i = tid; i < ny * mpr; i += TPB) {
            const int y = i / mpr, k = i - y * mpr;
            *(uint4 *)(mask_out + ((long long)b * S + y0 + y) * S + X0 + 16 * k) = *(const uint4 *)(sMsk + y * TX + 16 * k);
        }
    } else {
        for (int i = tid; i < ny * nx * 3; i += TPB) {
            const int y = i / (nx * 3), k = i - y * nx * 3;
            img_out[(((long long)b * S + y0 + y) * S + X0) * 3 + k] = sImg[y * TX * 3 + k];
        }
        for (int i = tid; i < ny * nx; i += TPB) {
            const int y = i / nx, k = i - y * nx;
            mask_out[((long long)b * S + y0 + y) * S + X0 + k] = sMsk[y * TX + k];
        }
    }
}

// ---------------------------------------------------------------------------------------------------- colour jitter
struct Rgb {
    int r, g, b;
};
__device__ __forceinline__ int grey_of(Rgb p) { return (p.r * 19595 + p.g * 38470 + p.b * 7471 + 0x8000) >> 16; }     // PIL's convert("L")
// Image.blend(lo, v, alpha) in its C float arithmetic: (UINT8)(lo + alpha * (v - lo)), clipped where it extrapolates
__device__ __forceinline__ int blend(int lo, int v, float alpha)
{
    float t = __fadd_rn((float)lo, __fmul_rn(alpha, (float)(v - lo)));
    t = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);
    return (int)t;
}
__device__ __forceinline__ Rgb blend3(int lr, int lg, int lb, Rgb p, float alpha) { return {blend(lr, p.r, alpha), blend(lg, p.g, alpha), blend(lb, p.b, alpha)}; }
__device__ __forceinline__ int round8(double x) { return clip8((int)floor(x + 0.5)); }
// PIL's RGB -> HSV, H += shift (mod 256), HSV -> RGB, in the float / double mixture of its Convert.c
__device__ __noinline__ Rgb hue_shift(Rgb p, int shift)
{
    const int maxc = max(p.r, max(p.g, p.b)), minc = min(p.r, min(p.g, p.b));
    int uh = 0, us = 0;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - p.r) / cr, gc = (float)(maxc - p.g) / cr, bc = (float)(maxc - p.b) / cr;
        float h;
        if (p.r == maxc) h = (float)(double)(bc - gc);
        else if (p.g == maxc) h = (float)((2.0 + (double)rc) - (double)bc);
        else h = (float)((4.0 + (double)gc) - (double)rc);
        const double t = (double)h / 6.0 + 1.0;
        h = (float)(t - floor(t));
        uh = clip8((int)((double)h * 255.0));
        us = clip8((int)((double)s * 255.0));
    }
    uh = (uh + shift) & 255;
    if (us == 0) return {maxc, maxc, maxc};
    const double h6 = (double)(float)uh * 6.0 / 255.0;
    const double fi = floor(h6);
    const float f = (float)(h6 - (double)(float)fi);
    const float fs = (float)((double)(float)us / 255.0);
    const double v = (double)(float)maxc;
    const int pp = round8(v * (1.0 - (double)fs));
    const int q = round8(v * (1.0 - (double)(fs * f)));
    const int t = round8(v * (1.0 - (double)fs * (1.0 - (double)f)));
    switch ((int)fi % 6) {
    case 0: return {maxc, t, pp};
    case 1: return {q, maxc, pp};
    case 2: return {pp, maxc, t};
    case 3: return {pp, q, maxc};
    case 4: return {t, pp, maxc};
    default: return {maxc, pp, q};
    }
}
__device__ __forceinline__ Rgb apply_op(int op, Rgb p, const int32_t *row, int mean)
{
    switch (op) {
    case OP_BRIGHTNESS: return blend3(0, 0, 0, p, __int_as_float(row[I_FB]));
    case OP_CONTRAST: return blend3(mean, mean, mean, p, __int_as_float(row[I_FC]));
    case OP_SATURATION: {
        const int g = grey_of(p);
        return blend3(g, g, g, p, __int_as_float(row[I_FS]));
    }
    case OP_HUE: return hue_shift(p, row[I_HUE] & 255);
    default: return p;
    }
}

// POST false: the operations in front of contrast, written back when there are any, and the sample's grey sum into sums[b].
// POST true: contrast against the mean of that sum, then the operations behind it.  P pixels a thread.
template <int P, bool POST>
__global__ __launch_bounds__(TPB) void seg_jitter_kernel(uint8_t *__restrict__ img, const int32_t *__restrict__ params, long long pld, long long pixels,
                                                         long long chunks, unsigned long long *__restrict__ sums)
{
    __shared__ unsigned int sPart[TPB / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int32_t *row = params + b * pld;
    if (!row[I_JITTER]) return;
    int pos = 4;
    for (int k = 3; k >= 0; --k)
        if (row[I_ORDER + k] == OP_CONTRAST) pos = k;
    const long long i = (long long)blockIdx.x * TPB + tid;
    const bool active = i < chunks;
    uint8_t *p = img + ((long long)b * pixels + i * P) * 3;
    alignas(16) uint8_t v[P * 3];
    unsigned int part = 0;
    if (active) {
        if constexpr (P == 1) v[0] = p[0], v[1] = p[1], v[2] = p[2];
        else
            for (int k = 0; k < P * 3 / 16; ++k) ((uint4 *)v)[k] = ((const uint4 *)p)[k];
        int mean = 0;
        if constexpr (POST) {
            const unsigned long long total = sums[b], count = (unsigned long long)pixels;
            mean = (int)((2 * total + count) / (2 * count));        // int(sum / N + 0.5), exactly
        }
#pragma unroll
        for (int k = 0; k < P; ++k) {
            Rgb c = {v[3 * k], v[3 * k + 1], v[3 * k + 2]};
            if constexpr (!POST) {
                for (int o = 0; o < pos; ++o) c = apply_op(row[I_ORDER + o], c, row, 0);
                part += (unsigned int)grey_of(c);
            } else {
                for (int o = pos; o < 4; ++o) c = apply_op(row[I_ORDER + o], c, row, mean);
            }
            v[3 * k] = (uint8_t)c.r, v[3 * k + 1] = (uint8_t)c.g, v[3 * k + 2] = (uint8_t)c.b;
        }
        if (POST || pos > 0) {
            if constexpr (P == 1) p[0] = v[0], p[1] = v[1], p[2] = v[2];
            else
                for (int k = 0; k < P * 3 / 16; ++k) ((uint4 *)p)[k] = ((const uint4 *)v)[k];
        }
    }
    if constexpr (!POST) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
        if ((tid & 63) == 0) sPart[tid >> 6] = part;
        __syncthreads();
        if (tid == 0) {
            unsigned long long s = 0;
            for (int k = 0; k < TPB / 64; ++k) s += sPart[k];
            atomicAdd(&sums[b], s);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- blur + quantise + normalise + layout
// One workgroup per TY x TX tile of one image.  T: the element's bits (uint32_t for fp32, uint16_t for bf16); V: elements a store.
template <typename T, bool NHWC, int V, bool BLUR>
__global__ __launch_bounds__(TPB) void seg_finish_kernel(const uint8_t *__restrict__ img, const uint8_t *__restrict__ mask, long long n, int H, int W,
                                                         const int32_t *__restrict__ params, long long pld, int use_index, int src_vec,
                                                         const T *__restrict__ table, T *__restrict__ out, int ld, int64_t *__restrict__ mask_out)
{
    constexpr int AW = TX + 2 * RMAX, AH = TY + 2 * RMAX;
    __shared__ alignas(16) uint8_t sRes[TY * TX * 3];
    __shared__ alignas(16) uint8_t sMsk[TY * TX];
    __shared__ double sA[BLUR ? AH * AW * 3 : 1], sB[BLUR ? TY * AW * 3 : 1], sW[RMAX + 1];
    const int tid = threadIdx.x, b = blockIdx.z, x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    const int nx = min(TX, W - x0), ny = min(TY, H - y0);
    const int32_t *row = params + b * pld;
    const long long idx = use_index ? sample_index(row, n) : b;
    const uint8_t *src = img + idx * H * W * 3;
    const uint8_t *msrc = mask + idx * H * W;
    int radius = 0;
    if constexpr (BLUR) radius = min(max(row[I_RADIUS], 0), RMAX);

    if (BLUR && radius > 0) {
        if constexpr (BLUR) {
            if (tid <= RMAX) sW[tid] = __hiloint2double(row[I_WEIGHTS + 2 * tid + 1], row[I_WEIGHTS + 2 * tid]);
            const double *w = sW;
            const int aw = nx + 2 * radius, ah = ny + 2 * radius;
            for (int i = tid; i < ah * aw * 3; i += TPB) {
                const int c = i % 3, ax = i / 3 % aw, ay = i / (3 * aw);
                const int sy = min(max(y0 + ay - radius, 0), H - 1), sx = min(max(x0 + ax - radius, 0), W - 1);      // mode='nearest'
                sA[(ay * AW + ax) * 3 + c] = (double)src[((long long)sy * W + sx) * 3 + c] / 255.0;
            }
            __syncthreads();
            for (int i = tid; i < ny * aw * 3; i += TPB) {                               // along the rows (axis 0) first, as scipy
                const int k = i % (aw * 3), y = i / (aw * 3);
                const double *q = sA + (y + radius) * AW * 3 + k;
                double acc = q[0] * w[0];
                for (int j = radius; j >= 1; --j) acc = acc + (q[-j * AW * 3] + q[j * AW * 3]) * w[j];
                sB[y * AW * 3 + k] = acc;
            }
            __syncthreads();
            for (int i = tid; i < ny * nx * 3; i += TPB) {
                const int c = i % 3, x = i / 3 % nx, y = i / (3 * nx);
                const double *q = sB + (y * AW + x + radius) * 3 + c;
                double acc = q[0] * w[0];
                for (int j = radius; j >= 1; --j) acc = acc + (q[-3 * j] + q[3 * j]) * w[j];
                double t = acc * 255.0;
                t = t < 0.0 ? 0.0 : (t > 255.0 ? 255.0 : t);
                sRes[(y * TX + x) * 3 + c] = (uint8_t)(int)t;                            // .astype(np.uint8): truncation
            }
        }
    } else if (src_vec) {           // W % 32 == 0: a whole tile row is 96 aligned bytes
        for (int i = tid; i < ny * 6; i += TPB) {
            const int y = i / 6, k = i - y * 6;
            ((uint4 *)sRes)[y * 6 + k] = *(const uint4 *)(src + ((long long)(y0 + y) * W + x0) * 3 + 16 * k);
        }
    } else {
        for (int i = tid; i < ny * nx * 3; i += TPB) {
            const int y = i / (nx * 3), k = i - y * nx * 3;
            sRes[y * TX * 3 + k] = src[((long long)(y0 + y) * W + x0) * 3 + k];
        }
    }
    if (src_vec) {
        for (int i = tid; i < ny * 2; i += TPB) ((uint4 *)sMsk)[i] = *(const uint4 *)(msrc + (long long)(y0 + (i >> 1)) * W + x0 + 16 * (i & 1));
    } else {
        for (int i = tid; i < ny * nx; i += TPB) sMsk[i / nx * TX + i % nx] = msrc[(long long)(y0 + i / nx) * W + x0 + i % nx];
    }
    __syncthreads();

    if constexpr (!NHWC) {
        const int ppr = nx / V;     // V > 1: W % V == 0, so nx is whole pieces
        for (int i = tid; i < 3 * ny * ppr; i += TPB) {
            const int k = i % ppr, y = i / ppr % ny, c = i / (ppr * ny);
            alignas(16) T v[V];
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = table[c * 256 + sRes[(y * TX + k * V + j) * 3 + c]];
            T *dst = out + (((long long)b * 3 + c) * H + y0 + y) * W + x0 + k * V;
            if constexpr (V == 1) *dst = v[0];
            else *(uint4 *)dst = *(const uint4 *)v;
        }
    } else {
        const int ppr = nx * ld / V;    // V > 1: W * ld % V == 0 and 32 * ld % V == 0, so a tile row is whole pieces
        for (int i = tid; i < ny * ppr; i += TPB) {
            const int k = i % ppr, y = i / ppr;
            int pix = k * V / ld, c = k * V - pix * ld;
            alignas(16) T v[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                v[j] = c < 3 ? table[c * 256 + sRes[(y * TX + pix) * 3 + c]] : (T)0;
                if (++c == ld) c = 0, ++pix;
            }
            T *dst = out + (((long long)b * H + y0 + y) * W + x0) * ld + (long long)k * V;
            if constexpr (V == 1) *dst = v[0];
            else *(uint4 *)dst = *(const uint4 *)v;
        }
    }
    if constexpr (V == 1) {
        for (int i = tid; i < ny * nx; i += TPB) mask_out[((long long)b * H + y0 + i / nx) * W + x0 + i % nx] = sMsk[i / nx * TX + i % nx];
    } else {                        // W even: two labels a store
        const int ppr = nx / 2;
        for (int i = tid; i < ny * ppr; i += TPB) {
            const int k = i % ppr, y = i / ppr;
            alignas(16) int64_t m[2] = {sMsk[y * TX + 2 * k], sMsk[y * TX + 2 * k + 1]};
            *(uint4 *)(mask_out + ((long long)b * H + y0 + y) * W + x0 + 2 * k) = *(const uint4 *)m;
        }
    }
}

template <typename T, int VEC>
void launch_finish(const SegFinishSel &sel, int layout, int blur, const uint8_t *img, const uint8_t *mask, int64_t n, int H, int W, const int32_t *params,
                   int64_t pld, int use_index, const void *table, void *out, int ld, int64_t *mask_out, hipStream_t s)
{
    const dim3 grid(sel.gx, sel.gy, sel.gz), block(TPB);
    const T *t = (const T *)table;
    T *o = (T *)out;
#define SEG_FINISH(NHWC, V, BLUR)                                                                                                                  \
    hipLaunchKernelGGL((seg_finish_kernel<T, NHWC, V, BLUR>), grid, block, 0, s, img, mask, (long long)n, H, W, params, (long long)pld, use_index, \
                       sel.src_vec, t, o, ld, mask_out)
    const bool nhwc = layout == KD_SEG_NHWC, vec = sel.vec != 1;
    if (nhwc) {
        if (blur) { if (vec) SEG_FINISH(true, VEC, true); else SEG_FINISH(true, 1, true); }
        else { if (vec) SEG_FINISH(true, VEC, false); else SEG_FINISH(true, 1, false); }
    } else {
        if (blur) { if (vec) SEG_FINISH(false, VEC, true); else SEG_FINISH(false, 1, true); }
        else { if (vec) SEG_FINISH(false, VEC, false); else SEG_FINISH(false, 1, false); }
    }
#undef SEG_FINISH
}

}  // namespace

extern "C" int kd_seg_crop(const uint8_t *data, const uint8_t *targets, int64_t n, int32_t H, int32_t W, const int32_t *params, int64_t params_ld,
                           int32_t B, int32_t S, uint8_t *img_out, uint8_t *mask_out, kd_stream_t stream)
{
    KD_REQUIRE(data && targets && params && img_out && mask_out, KD_ERR_INVALID, "kd_seg_crop: null argument");
    KD_REQUIRE(n >= 1 && n <= INT32_MAX, KD_ERR_INVALID, "kd_seg_crop: a dataset of %lld images", (long long)n);
    KD_REQUIRE(seg_side_ok(H) && seg_side_ok(W) && seg_side_ok(S), KD_ERR_UNSUPPORTED, "kd_seg_crop: H = %d, W = %d, S = %d outside [1, %d]", (int)H,
               (int)W, (int)S, SEG_MAX_SIDE);
    KD_REQUIRE(seg_batch_ok(B), KD_ERR_UNSUPPORTED, "kd_seg_crop: a batch of %d samples, 1 to %d", (int)B, SEG_MAX_BATCH);
    KD_REQUIRE(params_ld >= seg_row_words(S), KD_ERR_INVALID, "kd_seg_crop: parameter rows of %lld words, %lld needed for S = %d", (long long)params_ld,
               seg_row_words(S), (int)S);
    KD_REQUIRE(((uintptr_t)params & 3) == 0 && ((uintptr_t)data & 3) == 0, KD_ERR_INVALID, "kd_seg_crop: data or params is not aligned to 4 bytes");
    const SegCropSel sel = seg_crop_select(img_out, mask_out, B, S);
    KD_NOTE_PLUMBING(seg_kernel_name(sel.kernel));
    const dim3 grid(sel.gx, sel.gy, sel.gz), block(TPB);
    hipStream_t s = (hipStream_t)stream;
    if (sel.store == 16)
        hipLaunchKernelGGL((seg_crop_kernel<16>), grid, block, 0, s, data, targets, (long long)n, H, W, params, (long long)params_ld, S, img_out, mask_out);
    else hipLaunchKernelGGL((seg_crop_kernel<1>), grid, block, 0, s, data, targets, (long long)n, H, W, params, (long long)params_ld, S, img_out, mask_out);
    KD_CHECK_LAUNCH("kd_seg_crop");
    return KD_OK;
}

extern "C" size_t kd_seg_jitter_workspace(int32_t B) { return seg_jitter_workspace(B); }

extern "C" int kd_seg_jitter(uint8_t *img, const int32_t *params, int64_t params_ld, int32_t B, int32_t S, void *workspace, size_t workspace_bytes,
                             kd_stream_t stream)
{
    KD_REQUIRE(img && params && workspace, KD_ERR_INVALID, "kd_seg_jitter: null argument");
    KD_REQUIRE(seg_side_ok(S), KD_ERR_UNSUPPORTED, "kd_seg_jitter: S = %d outside [1, %d]", (int)S, SEG_MAX_SIDE);
    KD_REQUIRE(seg_batch_ok(B), KD_ERR_UNSUPPORTED, "kd_seg_jitter: a batch of %d samples, 1 to %d", (int)B, SEG_MAX_BATCH);
    KD_REQUIRE(params_ld >= SEG_HDR, KD_ERR_INVALID, "kd_seg_jitter: parameter rows of %lld words, %d at least", (long long)params_ld, SEG_HDR);
    KD_REQUIRE(((uintptr_t)params & 3) == 0 && ((uintptr_t)workspace & 7) == 0, KD_ERR_INVALID, "kd_seg_jitter: params or workspace is misaligned");
    KD_REQUIRE(workspace_bytes >= seg_jitter_workspace(B), KD_ERR_WORKSPACE, "kd_seg_jitter: workspace of %zu bytes, %zu needed", workspace_bytes,
               seg_jitter_workspace(B));
    const SegJitterSel sel = seg_jitter_select(img, B, S);
    KD_NOTE_PLUMBING(seg_kernel_name(sel.kernel));
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *sums = (unsigned long long *)workspace;
    if (hipMemsetAsync(sums, 0, seg_jitter_workspace(B), s) != hipSuccess) {
        kd_set_error("kd_seg_jitter: clearing the workspace failed");
        return KD_ERR_HIP;
    }
    const dim3 grid(sel.gx, sel.gy), block(TPB);
    const long long pixels = (long long)S * S;
    if (sel.pixels == 1) {
        hipLaunchKernelGGL((seg_jitter_kernel<1, false>), grid, block, 0, s, img, params, (long long)params_ld, pixels, sel.chunks, sums);
        hipLaunchKernelGGL((seg_jitter_kernel<1, true>), grid, block, 0, s, img, params, (long long)params_ld, pixels, sel.chunks, sums);
    } else {
        hipLaunchKernelGGL((seg_jitter_kernel<SEG_JITTER_PIXELS, false>), grid, block, 0, s, img, params, (long long)params_ld, pixels, sel.chunks, sums);
        hipLaunchKernelGGL((seg_jitter_kernel<SEG_JITTER_PIXELS, true>), grid, block, 0, s, img, params, (long long)params_ld, pixels, sel.chunks, sums);
    }
    KD_CHECK_LAUNCH("kd_seg_jitter");
    return KD_OK;
}

extern "C" int kd_seg_finish(const uint8_t *img, const uint8_t *mask, int64_t n, int32_t H, int32_t W, const int32_t *params, int64_t params_ld,
                             int32_t B, int32_t use_index, int32_t blur, const void *table, int32_t dtype, int32_t layout, void *out, int32_t ld,
                             int64_t *mask_out, kd_stream_t stream)
{
    KD_REQUIRE(img && mask && params && table && out && mask_out, KD_ERR_INVALID, "kd_seg_finish: null argument");
    KD_REQUIRE(seg_dtype_ok(dtype), KD_ERR_INVALID, "kd_seg_finish: dtype %d is neither KD_F32 nor KD_BF16", (int)dtype);
    KD_REQUIRE(seg_layout_ok(layout), KD_ERR_INVALID, "kd_seg_finish: layout %d is neither KD_SEG_NCHW nor KD_SEG_NHWC", (int)layout);
    KD_REQUIRE(n >= 1 && n <= INT32_MAX, KD_ERR_INVALID, "kd_seg_finish: %lld source images", (long long)n);
    KD_REQUIRE(use_index || n >= B, KD_ERR_INVALID, "kd_seg_finish: %lld source images for a batch of %d", (long long)n, (int)B);
    KD_REQUIRE(seg_side_ok(H) && seg_side_ok(W), KD_ERR_UNSUPPORTED, "kd_seg_finish: H = %d, W = %d outside [1, %d]", (int)H, (int)W, SEG_MAX_SIDE);
    KD_REQUIRE(seg_batch_ok(B), KD_ERR_UNSUPPORTED, "kd_seg_finish: a batch of %d samples, 1 to %d", (int)B, SEG_MAX_BATCH);
    KD_REQUIRE(layout != KD_SEG_NHWC || (ld >= SEG_CH && ld <= 4096), KD_ERR_INVALID, "kd_seg_finish: pixel stride %d outside [3, 4096]", (int)ld);
    KD_REQUIRE(params_ld >= SEG_HDR, KD_ERR_INVALID, "kd_seg_finish: parameter rows of %lld words, %d at least", (long long)params_ld, SEG_HDR);
    KD_REQUIRE(((uintptr_t)out & (seg_elem_size(dtype) - 1)) == 0 && ((uintptr_t)table & (seg_elem_size(dtype) - 1)) == 0 &&
                   ((uintptr_t)params & 3) == 0 && ((uintptr_t)mask_out & 7) == 0,
               KD_ERR_INVALID, "kd_seg_finish: an operand is not aligned to its element");
    const SegFinishSel sel = seg_finish_select(dtype, layout, blur != 0, img, mask, out, mask_out, B, H, W, ld);
    KD_NOTE_PLUMBING(seg_kernel_name(sel.kernel));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == KD_BF16) launch_finish<uint16_t, 8>(sel, layout, blur != 0, img, mask, n, H, W, params, params_ld, use_index, table, out, ld, mask_out, s);
    else launch_finish<uint32_t, 4>(sel, layout, blur != 0, img, mask, n, H, W, params, params_ld, use_index, table, out, ld, mask_out, s);
    KD_CHECK_LAUNCH("kd_seg_finish");
    return KD_OK;
}
