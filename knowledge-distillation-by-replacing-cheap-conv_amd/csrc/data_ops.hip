// One training batch of CIFAR from the device-resident dataset in one launch (kd_cifar_batch): RandomCrop(32, padding=4),
// RandomHorizontalFlip, ToTensor and Normalize of the reference's loaders (data_loader/data_loaders.py:13-53), whose random draws
// arrive as a per-image row [index, dy, dx, flip] and whose arithmetic arrives as a 3 x 256 table in the output's dtype.  The kernel
// is a pure gather: output element (b, c, y, x) is table[c][byte] of source pixel (y + dy - 4, x' + dx - 4), x' = flip ? 31 - x : x,
// and table[c][0] -- the normalised value of the 0 the reference pads with -- outside the image.  It moves bits and computes no
// value, so it agrees bit for bit with the host composition that built the table.  The labels are gathered by the first B threads.
//
// A thread owns V consecutive elements of the output's storage (V = 1, or 16 B of them: one store); consecutive threads own
// consecutive pieces, so a wave's stores are one contiguous run.  NCHW: a piece is V pixels of one row of one plane.  NHWC: the
// kernel owns every pixel's whole stride ld, channels [3, ld) are its zeros, so the storage is one dense run whatever ld is and a
// piece may straddle pixels.  Which instantiation runs is data_select.h's decision; the launcher below only launches.
#include "data_select.h"
#include "kd_common.h"

namespace {

constexpr int TPB = DATA_TPB, SIDE = DATA_SIDE, CH = DATA_CH, PIXELS = DATA_PIXELS, PAD = DATA_PAD;

// table[c][byte] of the source pixel of output (c, y, x) for the image that row q = [index, dy, dx, flip] describes.  A row outside
// its ranges reads nothing: every pixel of that image is padding.
template <typename T>
__device__ __forceinline__ T gather(const uint8_t *__restrict__ data, long long n, const int32_t *__restrict__ q, const T *__restrict__ table, int c,
                                    int y, int x)
{
    const int idx = q[0], dy = q[1], dx = q[2], flip = q[3];
    const int sy = y + dy - PAD, sx = (flip ? SIDE - 1 - x : x) + dx - PAD;
    const bool row_ok = idx >= 0 && idx < n && dy >= 0 && dy <= 2 * PAD && dx >= 0 && dx <= 2 * PAD;
    const bool inside = row_ok && sy >= 0 && sy < SIDE && sx >= 0 && sx < SIDE;
    const int byte = inside ? data[((long long)idx * PIXELS + sy * SIDE + sx) * CH + c] : 0;
    return table[c * 256 + byte];
}

// T: the element's bits (uint32_t for fp32, uint16_t for bf16).  items = elements of the storage / V.
template <typename T, bool NHWC, int V>
__global__ __launch_bounds__(TPB) void cifar_batch_kernel(const uint8_t *__restrict__ data, const int64_t *__restrict__ labels, long long n,
                                                          const int32_t *__restrict__ params, int B, const T *__restrict__ table,
                                                          T *__restrict__ out, int ld, long long items, int64_t *__restrict__ labels_out)
{
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i < B) {        // (items >= B: an image is at least 3072 / 8 items)
        long long idx = params[4 * i];
        idx = idx < 0 ? 0 : (idx >= n ? n - 1 : idx);
        labels_out[i] = labels[idx];
    }
    if (i >= items) return;
    const long long f0 = i * V;
    alignas(16) T v[V];
    if constexpr (!NHWC) {
        const int x0 = (int)(f0 % SIDE), y = (int)(f0 / SIDE % SIDE), c = (int)(f0 / PIXELS % CH);
        const int32_t *q = params + 4 * (f0 / (PIXELS * CH));
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = gather<T>(data, n, q, table, c, y, x0 + j);
    } else {
        long long p = f0 / ld;
        int c = (int)(f0 - p * ld);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int pix = (int)(p % PIXELS);
            v[j] = c < CH ? gather<T>(data, n, params + 4 * (p / PIXELS), table, c, pix / SIDE, pix % SIDE) : (T)0;
            if (++c == ld) {
                c = 0;
                ++p;
            }
        }
    }
    if constexpr (V == 1) out[f0] = v[0];
    else *(uint4 *)(out + f0) = *(const uint4 *)v;
}

template <typename T, int VEC>
void launch(const DataSel &sel, int layout, const uint8_t *data, const int64_t *labels, int64_t n, const int32_t *params, int B, const void *table,
            void *out, int ld, int64_t *labels_out, hipStream_t s)
{
    const dim3 grid(sel.grid), block(TPB);
    const T *t = (const T *)table;
    T *o = (T *)out;
    if (layout == KD_CIFAR_NHWC) {
        if (sel.vec == 1) hipLaunchKernelGGL((cifar_batch_kernel<T, true, 1>), grid, block, 0, s, data, labels, (long long)n, params, B, t, o, ld, sel.items, labels_out);
        else hipLaunchKernelGGL((cifar_batch_kernel<T, true, VEC>), grid, block, 0, s, data, labels, (long long)n, params, B, t, o, ld, sel.items, labels_out);
    } else {
        if (sel.vec == 1) hipLaunchKernelGGL((cifar_batch_kernel<T, false, 1>), grid, block, 0, s, data, labels, (long long)n, params, B, t, o, ld, sel.items, labels_out);
        else hipLaunchKernelGGL((cifar_batch_kernel<T, false, VEC>), grid, block, 0, s, data, labels, (long long)n, params, B, t, o, ld, sel.items, labels_out);
    }
}

}  // namespace

extern "C" int kd_cifar_batch(const uint8_t *data, const int64_t *labels, int64_t n, const int32_t *params, int32_t B, const void *table,
                              int32_t dtype, int32_t layout, void *out, int32_t ld, int64_t *labels_out, kd_stream_t stream)
{
    KD_REQUIRE(data && labels && params && table && out && labels_out, KD_ERR_INVALID, "kd_cifar_batch: null argument");
    KD_REQUIRE(data_dtype_ok(dtype), KD_ERR_INVALID, "kd_cifar_batch: dtype %d is neither KD_F32 nor KD_BF16", (int)dtype);
    KD_REQUIRE(data_layout_ok(layout), KD_ERR_INVALID, "kd_cifar_batch: layout %d is neither KD_CIFAR_NCHW nor KD_CIFAR_NHWC", (int)layout);
    KD_REQUIRE(n >= 1 && n <= INT32_MAX, KD_ERR_INVALID, "kd_cifar_batch: a dataset of %lld images", (long long)n);
    KD_REQUIRE(B >= 1, KD_ERR_INVALID, "kd_cifar_batch: a batch of %d images", (int)B);
    KD_REQUIRE(layout != KD_CIFAR_NHWC || ld >= DATA_CH, KD_ERR_INVALID, "kd_cifar_batch: pixel stride %d below 3", (int)ld);
    KD_REQUIRE(data_shape_ok(layout, B, ld), KD_ERR_UNSUPPORTED, "kd_cifar_batch: B = %d, ld = %d is more than 2^31 output elements", (int)B, (int)ld);
    KD_REQUIRE(((uintptr_t)out & (data_elem_size(dtype) - 1)) == 0 && ((uintptr_t)table & (data_elem_size(dtype) - 1)) == 0 &&
                   ((uintptr_t)params & 3) == 0 && ((uintptr_t)labels & 7) == 0 && ((uintptr_t)labels_out & 7) == 0,
               KD_ERR_INVALID, "kd_cifar_batch: an operand is not aligned to its element");
    const DataSel sel = data_select(dtype, layout, out, B, ld);
    KD_NOTE_PLUMBING(data_kernel_name(sel.kernel));
    hipStream_t s = (hipStream_t)stream;
    if (dtype == KD_BF16) launch<uint16_t, 8>(sel, layout, data, labels, n, params, B, table, out, ld, labels_out, s);
    else launch<uint32_t, 4>(sel, layout, data, labels, n, params, B, table, out, ld, labels_out, s);
    KD_CHECK_LAUNCH("kd_cifar_batch");
    return KD_OK;
}
