// DenseNet-BC CIFAR path (models/cifar_models/densenet.py): the memory-bound pieces around the MFMA convolutions of a dense
// block whose layers share one (N,H,W,C_end) NHWC buffer.
//
//   kd_bn_nhwc_stats / kd_bn_nhwc_apply: train-mode BatchNorm split in two.  The batch mean / variance of a channel of the block
//     buffer is the same for every later layer's norm1 (only gamma, beta and the running buffers differ), so the statistics are
//     reduced ONCE, when the 32-channel slice is produced, and each norm1 is then a single elementwise pass over its prefix.
//     The reduction and the normalise pass are kd_bn_nhwc_fwd's (bn_nhwc_core.h's bn_stats / bn_apply for float, chosen by
//     bn_select.h): per channel the same bits.
//   kd_avgpool2x2_nhwc / _bwd: the transition's AvgPool2d(2, 2) on NHWC views, floor output size (an odd last row / column is
//     dropped and gets zero gradient).  One thread per output (backward: input) pixel x 4 channels (float4) when bn_select.h's
//     bn_vec_ok(4, ...) allows it, else per channel; consecutive threads take consecutive channels, so a wave reads whole 256-B /
//     1-KiB runs of a pixel.
#include "bn_nhwc_core.h"

namespace {

// running statistics of one BN from supplied batch statistics: what bn_nhwc_stats_finish_kernel does for its own
__global__ void bn_nhwc_running_kernel(int C, const float *__restrict__ mean, const float *__restrict__ var_unb,
                                       float *__restrict__ run_mean, float *__restrict__ run_var, float momentum)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    if (run_mean) run_mean[c] = bn_running_update(run_mean[c], momentum, mean[c]);
    if (run_var) run_var[c] = bn_running_update(run_var[c], momentum, var_unb[c]);
}

struct PoolGeom {
    int N, H, W, C, Ho, Wo;
};

// y[n][ho][wo][c] = ((x[2ho][2wo] + x[2ho][2wo+1]) + (x[2ho+1][2wo] + x[2ho+1][2wo+1])) / 4
template <int V>
__global__ __launch_bounds__(TPB) void avgpool2x2_kernel(PoolGeom g, const float *__restrict__ x, int ldx, float *__restrict__ y, int ldy)
{
    const int cv = g.C / V;
    const long long total = (long long)g.N * g.Ho * g.Wo * cv;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const long long po = i / cv;                         // output pixel
        const int c0 = (int)(i - po * cv) * V;
        const int wo = (int)(po % g.Wo);
        const long long t = po / g.Wo;
        const int ho = (int)(t % g.Ho);
        const long long n = t / g.Ho;
        const long long pi = (n * g.H + 2 * ho) * g.W + 2 * wo;    // input pixel (2ho, 2wo); 2ho + 1 < H and 2wo + 1 < W
        float a[V], b[V], c[V], d[V], o[V];
        ldv<V>(x + pi * ldx + c0, a);
        ldv<V>(x + (pi + 1) * ldx + c0, b);
        ldv<V>(x + (pi + g.W) * ldx + c0, c);
        ldv<V>(x + (pi + g.W + 1) * ldx + c0, d);
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = ((a[j] + b[j]) + (c[j] + d[j])) * 0.25f;
        stv<V>(y + po * ldy + c0, o);
    }
}

// gx[n][h][w][c] = gy[h/2][w/2] / 4 inside the pooled area, 0 on a dropped last row / column
template <int V>
__global__ __launch_bounds__(TPB) void avgpool2x2_bwd_kernel(PoolGeom g, const float *__restrict__ gy, int ldg, float *__restrict__ gx, int ldgx)
{
    const int cv = g.C / V;
    const long long total = (long long)g.N * g.H * g.W * cv;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const long long pi = i / cv;                         // input pixel
        const int c0 = (int)(i - pi * cv) * V;
        const int w = (int)(pi % g.W);
        const long long t = pi / g.W;
        const int h = (int)(t % g.H);
        const long long n = t / g.H;
        float o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = 0.f;
        if (h < 2 * g.Ho && w < 2 * g.Wo) {
            float v[V];
            ldv<V>(gy + ((n * g.Ho + (h >> 1)) * g.Wo + (w >> 1)) * ldg + c0, v);
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = v[j] * 0.25f;
        }
        stv<V>(gx + pi * ldgx + c0, o);
    }
}

int pool_geom(int N, int H, int W, int C, PoolGeom &g, const char *who)
{
    KD_REQUIRE(N > 0 && H >= 2 && W >= 2 && C > 0, KD_ERR_INVALID, "%s: bad shape N=%d H=%d W=%d C=%d (a 2x2 window needs H, W >= 2)", who, N, H, W, C);
    KD_REQUIRE((long long)N * H * W < (1ll << 31), KD_ERR_UNSUPPORTED, "%s: more than 2^31 pixels", who);
    g.N = N; g.H = H; g.W = W; g.C = C; g.Ho = H / 2; g.Wo = W / 2;
    return KD_OK;
}

}  // namespace

extern "C" int kd_bn_nhwc_stats(const float *x, int32_t ldx, int64_t M, int32_t C, float *mean, float *invstd, float *var_unbiased,
                                float eps, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    BnGeom g;
    if (int rc = geom(M, C, g, "kd_bn_nhwc_stats")) return rc;
    KD_REQUIRE(x && mean && invstd && var_unbiased, KD_ERR_INVALID, "kd_bn_nhwc_stats: null argument");
    KD_REQUIRE(ldx >= C, KD_ERR_INVALID, "kd_bn_nhwc_stats: pixel stride below C");
    return bn_stats<float>("kd_bn_nhwc_stats", bn_select_fwd(4, x, ldx, nullptr, 0, M, C), g, x, ldx, mean, invstd, nullptr, nullptr, var_unbiased, 0.f,
                           eps, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int kd_bn_nhwc_apply(const float *x, int32_t ldx, float *y, int32_t ldy, int64_t M, int32_t C, const float *gamma,
                                const float *beta, const float *mean, const float *invstd, const float *var_unbiased,
                                float *running_mean, float *running_var, float momentum, int32_t relu, kd_stream_t stream)
{
    BnGeom g;
    if (int rc = geom(M, C, g, "kd_bn_nhwc_apply")) return rc;
    KD_REQUIRE(x && y && gamma && beta && mean && invstd, KD_ERR_INVALID, "kd_bn_nhwc_apply: null argument");
    KD_REQUIRE(ldx >= C && ldy >= C, KD_ERR_INVALID, "kd_bn_nhwc_apply: pixel stride below C");
    KD_REQUIRE(!running_var || var_unbiased, KD_ERR_INVALID, "kd_bn_nhwc_apply: running_var needs the unbiased batch variance");
    hipStream_t s = (hipStream_t)stream;
    if (running_mean || running_var) {
        hipLaunchKernelGGL(bn_nhwc_running_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, (int)C, mean, var_unbiased, running_mean,
                           running_var, momentum);
        KD_CHECK_LAUNCH("kd_bn_nhwc_apply(running)");
    }
    const BnSel sel = bn_select_fwd(4, x, ldx, y, ldy, M, C);
    KD_NOTE_PLUMBING(bn_kernel_name(sel.kernel));
    return bn_apply<float>("kd_bn_nhwc_apply", sel, g, x, ldx, y, ldy, gamma, beta, mean, invstd, relu, s);
}

extern "C" int kd_avgpool2x2_nhwc(const float *x, int32_t ldx, float *y, int32_t ldy, int32_t N, int32_t H, int32_t W, int32_t C,
                                  kd_stream_t stream)
{
    PoolGeom g;
    if (int rc = pool_geom(N, H, W, C, g, "kd_avgpool2x2_nhwc")) return rc;
    KD_REQUIRE(x && y, KD_ERR_INVALID, "kd_avgpool2x2_nhwc: null argument");
    KD_REQUIRE(ldx >= C && ldy >= C, KD_ERR_INVALID, "kd_avgpool2x2_nhwc: pixel stride below C");
    hipStream_t s = (hipStream_t)stream;
    const long long outs = (long long)N * g.Ho * g.Wo;
    if (bn_vec_ok(4, C, x, ldx, y, ldy)) {
        KD_NOTE_PLUMBING("avgpool2x2_kernel<4>");
        hipLaunchKernelGGL(avgpool2x2_kernel<4>, dim3(bn_grid(outs * (C / 4))), dim3(TPB), 0, s, g, x, ldx, y, ldy);
    } else {
        KD_NOTE_PLUMBING("avgpool2x2_kernel<1>");
        hipLaunchKernelGGL(avgpool2x2_kernel<1>, dim3(bn_grid(outs * C)), dim3(TPB), 0, s, g, x, ldx, y, ldy);
    }
    KD_CHECK_LAUNCH("kd_avgpool2x2_nhwc");
    return KD_OK;
}

extern "C" int kd_avgpool2x2_nhwc_bwd(const float *gy, int32_t ldg, float *gx, int32_t ldgx, int32_t N, int32_t H, int32_t W, int32_t C,
                                      kd_stream_t stream)
{
    PoolGeom g;
    if (int rc = pool_geom(N, H, W, C, g, "kd_avgpool2x2_nhwc_bwd")) return rc;
    KD_REQUIRE(gy && gx, KD_ERR_INVALID, "kd_avgpool2x2_nhwc_bwd: null argument");
    KD_REQUIRE(ldg >= C && ldgx >= C, KD_ERR_INVALID, "kd_avgpool2x2_nhwc_bwd: pixel stride below C");
    hipStream_t s = (hipStream_t)stream;
    const long long ins = (long long)N * H * W;
    if (bn_vec_ok(4, C, gy, ldg, gx, ldgx)) {
        KD_NOTE_PLUMBING("avgpool2x2_bwd_kernel<4>");
        hipLaunchKernelGGL(avgpool2x2_bwd_kernel<4>, dim3(bn_grid(ins * (C / 4))), dim3(TPB), 0, s, g, gy, ldg, gx, ldgx);
    } else {
        KD_NOTE_PLUMBING("avgpool2x2_bwd_kernel<1>");
        hipLaunchKernelGGL(avgpool2x2_bwd_kernel<1>, dim3(bn_grid(ins * C)), dim3(TPB), 0, s, g, gy, ldg, gx, ldgx);
    }
    KD_CHECK_LAUNCH("kd_avgpool2x2_nhwc_bwd");
    return KD_OK;
}
