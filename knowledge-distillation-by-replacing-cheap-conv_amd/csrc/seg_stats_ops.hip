// Per-tile class statistics of the device-resident Cityscapes label maps (include/kdcc.h: kd_seg_class_stats): for every image, every
// tile x tile tile of it and every class, the number of the class's pixels and the sums of their x and y relative to the tile's
// origin.  The class centroids of the reference's data_loader/uniform.py:47-78 (scipy's center_of_mass per tile and class) are
// sum // count of these, taken on the host (data_loader/uniform.py here).  Integer sums throughout, so the result does not depend
// on the order of accumulation and is the same bits from run to run and as ops.seg_class_stats on host tensors.
//
// A unit is `rows` consecutive rows of one tile; a workgroup walks units with the grid as its stride.  Within a unit a thread keeps
// the run of equal labels it is in (label, count, sum x, sum y relative to the unit's first row) in registers and adds it to its
// wave's uint32 partials in LDS when the label changes -- label maps are mostly long runs -- and a chunk of 16 labels that continues
// the run is four compares.  After the unit the partials of the four waves are summed and every non-zero one goes to `stats` as one
// 64-bit atomic add.  seg_stats_select.h sizes `rows` so that the uint32 partials cannot overflow, and decides the variant and grid.
#include <limits.h>

#include "kd_common.h"
#include "seg_stats_select.h"

namespace {

constexpr int TPB = SEG_STATS_TPB, WAVES = TPB / 64, SLOTS = SEG_STATS_MAX_CLASSES * 3;

struct Run {
    unsigned lab, cnt, sx, sy;
};
__device__ __forceinline__ void run_flush(unsigned *part, int C, const Run &r)
{
    if (r.cnt && r.lab < (unsigned)C) {
        atomicAdd(&part[r.lab * 3], r.cnt);
        atomicAdd(&part[r.lab * 3 + 1], r.sx);
        atomicAdd(&part[r.lab * 3 + 2], r.sy);
    }
}
__device__ __forceinline__ void run_add(unsigned *part, int C, Run &r, unsigned lab, unsigned x, unsigned y)
{
    if (lab == r.lab) {
        r.cnt += 1, r.sx += x, r.sy += y;
    } else {
        run_flush(part, C, r);
        r.lab = lab, r.cnt = 1, r.sx = x, r.sy = y;
    }
}

// V: labels a thread loads at once.  V == 16: targets is 16-B aligned, W and tile are multiples of 16.
template <int V>
__global__ __launch_bounds__(TPB) void seg_class_stats_kernel(const uint8_t *__restrict__ targets, int H, int W, int tile, int C, int th, int tw,
                                                              int rows, int chunks, long long units, unsigned long long *__restrict__ stats)
{
    __shared__ unsigned sPart[WAVES * SLOTS];
    const int tid = threadIdx.x;
    unsigned *part = sPart + (tid >> 6) * SLOTS;
    const int per = tile / V;       // loads per row of a tile
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        long long t = u / chunks;
        const int ch = (int)(u - t * chunks);
        const int tx = (int)(t % tw);
        t /= tw;
        const int ty = (int)(t % th);
        const long long img = t / th;
        const int row0 = ch * rows, nr = min(rows, tile - row0);
        for (int i = tid; i < WAVES * SLOTS; i += TPB) sPart[i] = 0u;
        __syncthreads();
        // rows ty * tile + row0 + [0, nr) < th * tile <= H, columns tx * tile + [0, tile) < tw * tile <= W: inside image img
        const uint8_t *base = targets + ((img * H + (long long)ty * tile + row0) * W + (long long)tx * tile);
        const int total = nr * per;     // rows * tile <= max(SEG_STATS_WG_BYTES, tile)
        Run run = {256u, 0u, 0u, 0u};
        for (int e = tid; e < total; e += TPB) {
            const int r = e / per, x0 = (e - r * per) * V;
            const uint8_t *p = base + (long long)r * W + x0;
            if constexpr (V == 16) {
                const uint4 v = *(const uint4 *)p;
                const unsigned rep = (run.lab & 255u) * 0x01010101u;
                if (run.lab < 256u && v.x == rep && v.y == rep && v.z == rep && v.w == rep) {     // the run goes on: x0 .. x0 + 15
                    run.cnt += 16u, run.sx += 16u * (unsigned)x0 + 120u, run.sy += 16u * (unsigned)r;
                } else {
                    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int j = 0; j < 16; ++j) run_add(part, C, run, (w[j >> 2] >> (8 * (j & 3))) & 255u, (unsigned)(x0 + j), (unsigned)r);
                }
            } else {
                run_add(part, C, run, p[0], (unsigned)x0, (unsigned)r);
            }
        }
        run_flush(part, C, run);
        __syncthreads();
        unsigned long long *dst = stats + (((img * th + ty) * tw + tx) * C) * 3;
        for (int i = tid; i < C * 3; i += TPB) {
            const int c = i / 3, k = i - 3 * c;
            unsigned long long v = 0, cnt = 0;
            for (int w = 0; w < WAVES; ++w) v += sPart[w * SLOTS + i], cnt += sPart[w * SLOTS + 3 * c];
            if (k == 2) v += cnt * (unsigned long long)row0;        // y relative to the tile's origin
            if (v) atomicAdd(&dst[i], v);
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int kd_seg_class_stats(const uint8_t *targets, int64_t n, int32_t H, int32_t W, int32_t tile, int32_t num_classes, int64_t *stats,
                                  kd_stream_t stream)
{
    KD_REQUIRE(targets, KD_ERR_INVALID, "kd_seg_class_stats: null argument");
    KD_REQUIRE(n >= 1 && n <= INT32_MAX, KD_ERR_INVALID, "kd_seg_class_stats: a dataset of %lld images", (long long)n);
    KD_REQUIRE(seg_side_ok(H) && seg_side_ok(W), KD_ERR_UNSUPPORTED, "kd_seg_class_stats: H = %d, W = %d outside [1, %d]", (int)H, (int)W, SEG_MAX_SIDE);
    KD_REQUIRE(tile >= 1, KD_ERR_INVALID, "kd_seg_class_stats: a tile of %d pixels", (int)tile);
    KD_REQUIRE(seg_stats_classes_ok(num_classes), KD_ERR_UNSUPPORTED, "kd_seg_class_stats: 1 <= num_classes <= %d (got %d)", SEG_STATS_MAX_CLASSES,
               (int)num_classes);
    const SegStatsSel sel = seg_stats_select(targets, n, H, W, tile);
    if (!sel.launch) return KD_OK;      // a tile larger than the image: `stats` has no element
    KD_REQUIRE(stats && ((uintptr_t)stats & 7) == 0, KD_ERR_INVALID, "kd_seg_class_stats: stats is null or not aligned to 8 bytes");
    KD_NOTE_PLUMBING(seg_stats_kernel_name(sel.kernel));
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = (size_t)n * sel.th * sel.tw * num_classes * 3 * sizeof(int64_t);
    if (hipMemsetAsync(stats, 0, bytes, s) != hipSuccess) {
        kd_set_error("kd_seg_class_stats: clearing stats failed");
        return KD_ERR_HIP;
    }
    const dim3 grid(sel.grid), block(TPB);
    unsigned long long *out = (unsigned long long *)stats;
    if (sel.vec == 16)
        hipLaunchKernelGGL((seg_class_stats_kernel<16>), grid, block, 0, s, targets, H, W, tile, num_classes, sel.th, sel.tw, sel.rows, sel.chunks,
                           sel.units, out);
    else
        hipLaunchKernelGGL((seg_class_stats_kernel<1>), grid, block, 0, s, targets, H, W, tile, num_classes, sel.th, sel.tw, sel.rows, sel.chunks,
                           sel.units, out);
    KD_CHECK_LAUNCH("kd_seg_class_stats");
    return KD_OK;
}
