// BatchNorm2d on NHWC fp32 views for the Wide-ResNet-28-10 CIFAR path (models/cifar_models/wrn.py): 16 / 160 / 320 / 640
// channels at 32x32 .. 8x8, the student in TRAINING mode (classification_trainer.py:21) so every BN of it -- frozen
// ones included -- normalises with batch statistics between two MFMA convolutions.
//
// Every reduction is two fixed-order stages and no atomics, so results are bit-reproducible run to run:
//   stage 1 (one workgroup per ROWS pixels x 64 channels): per-block partials; in the forward the block sums x - k and
//           (x - k)^2 around k = the block's first pixel, so the fp32 sums see values of the order of the spread, not of the
//           mean (no E[x^2] - E[x]^2 cancellation when |mean| >> std);
//   stage 2: row-interleaved fp64 chains merged in a fixed order -- forward: 16 channels x 16 chains per workgroup, Chan's
//           pairwise update for mean / M2 and a fixed tree over the chains; backward: 64 channels x 4 chains, plain sums.
// The elementwise pass is a separate grid-stride kernel: y = relu?((x - mean) * gamma * invstd + beta), resp. dx.
#include "bn_nhwc_core.h"

namespace {

// stage 1 backward: part[rb][0][c] = sum g', part[rb][1][c] = sum g' * xhat (g' = relu ? g * [y > 0] : g)
__global__ __launch_bounds__(TPB) void bn_nhwc_grad_partial_kernel(BnGeom g, const float *__restrict__ gy, int ldg,
                                                                   const float *__restrict__ x, int ldx, const float *__restrict__ y,
                                                                   int ldy, const float *__restrict__ mean,
                                                                   const float *__restrict__ invstd, int relu, float *__restrict__ part)
{
    __shared__ float sh[2][4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + tx, rb = blockIdx.x;
    const long long r0 = (long long)rb * ROWS;
    const long long r1 = r0 + ROWS < g.M ? r0 + ROWS : g.M;
    float s1 = 0.f, s2 = 0.f;
    if (c < g.C) {
        const float mu = mean[c], is = invstd[c];
        for (long long r = r0 + ty; r < r1; r += 4) {
            const float gv = (relu && !(y[r * ldy + c] > 0.f)) ? 0.f : gy[r * ldg + c];
            s1 += gv;
            s2 = fmaf(gv, (x[r * ldx + c] - mu) * is, s2);
        }
    }
    sh[0][ty][tx] = s1;
    sh[1][ty][tx] = s2;
    __syncthreads();
    if (ty == 0 && c < g.C) {
        float *p = part + (size_t)rb * 2 * g.C;
        p[c] = (sh[0][0][tx] + sh[0][1][tx]) + (sh[0][2][tx] + sh[0][3][tx]);
        p[g.C + c] = (sh[1][0][tx] + sh[1][1][tx]) + (sh[1][2][tx] + sh[1][3][tx]);
    }
}

// stage 2 backward: sums[0][c] = sum g', sums[1][c] = sum g' * xhat (fp64 chains); dbeta / dgamma (+)= them when given
__global__ __launch_bounds__(TPB) void bn_nhwc_grad_finish_kernel(BnGeom g, const float *__restrict__ part, float *__restrict__ sums,
                                                                  float *__restrict__ dgamma, float *__restrict__ dbeta, int accumulate)
{
    __shared__ double sh[2][4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + tx;
    double a = 0.0, b = 0.0;
    if (c < g.C)
        for (int rb = ty; rb < g.nrb; rb += 4) {
            a += (double)part[(size_t)rb * 2 * g.C + c];
            b += (double)part[(size_t)rb * 2 * g.C + g.C + c];
        }
    sh[0][ty][tx] = a;
    sh[1][ty][tx] = b;
    __syncthreads();
    if (ty != 0 || c >= g.C) return;
    const float s1 = (float)((sh[0][0][tx] + sh[0][1][tx]) + (sh[0][2][tx] + sh[0][3][tx]));
    const float s2 = (float)((sh[1][0][tx] + sh[1][1][tx]) + (sh[1][2][tx] + sh[1][3][tx]));
    sums[c] = s1;
    sums[g.C + c] = s2;
    if (dbeta) dbeta[c] = accumulate ? dbeta[c] + s1 : s1;
    if (dgamma) dgamma[c] = accumulate ? dgamma[c] + s2 : s2;
}

// dx = gamma * invstd * (g' - [training] (sum g' + xhat * sum g' xhat) / M) + res
template <int V>
__global__ __launch_bounds__(TPB) void bn_nhwc_dx_kernel(BnGeom g, const float *__restrict__ gy, int ldg, const float *__restrict__ x,
                                                         int ldx, const float *__restrict__ y, int ldy, const float *__restrict__ res,
                                                         int ldres, float *__restrict__ dx, int lddx, const float *__restrict__ gamma,
                                                         const float *__restrict__ mean, const float *__restrict__ invstd,
                                                         const float *__restrict__ sums, int training, int relu)
{
    const int cv = g.C / V;
    const long long total = g.M * cv;
    const float inv_m = (float)(1.0 / (double)g.M);
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const long long m = i / cv;
        const int c0 = (int)(i - m * cv) * V;
        float gv[V], xv[V], yv[V], rv[V];
        auto load = [&](const float *p, long long off, float(&v)[V]) {
            if constexpr (V == 4) {
                const float4 a = *(const float4 *)(p + off);
                v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
            } else {
                v[0] = p[off];
            }
        };
        load(gy, m * ldg + c0, gv);
        if (training) load(x, m * ldx + c0, xv);
        if (relu) load(y, m * ldy + c0, yv);
        if (res) load(res, m * ldres + c0, rv);
        float o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int c = c0 + j;
            const float is = invstd[c];
            float t = (relu && !(yv[j] > 0.f)) ? 0.f : gv[j];
            if (training) t = t - sums[c] * inv_m - (xv[j] - mean[c]) * is * (sums[g.C + c] * inv_m);
            o[j] = gamma[c] * is * t;
            if (res) o[j] += rv[j];
        }
        if constexpr (V == 4) *(float4 *)(dx + m * lddx + c0) = make_float4(o[0], o[1], o[2], o[3]);
        else dx[m * lddx + c0] = o[0];
    }
}


}  // namespace

extern "C" size_t kd_bn_nhwc_workspace(int64_t M, int32_t C)
{
    return bn_workspace_bytes(M, C);
}

extern "C" int kd_bn_nhwc_fwd(const float *x, int32_t ldx, float *y, int32_t ldy, int64_t M, int32_t C, const float *gamma,
                              const float *beta, float *save_mean, float *save_invstd, float *running_mean, float *running_var,
                              float momentum, float eps, int32_t training, int32_t relu, void *workspace, size_t workspace_bytes,
                              kd_stream_t stream)
{
    BnGeom g;
    if (int rc = geom(M, C, g, "kd_bn_nhwc_fwd")) return rc;
    KD_REQUIRE(x && y && gamma && beta && save_mean && save_invstd, KD_ERR_INVALID, "kd_bn_nhwc_fwd: null argument");
    KD_REQUIRE(ldx >= C && ldy >= C, KD_ERR_INVALID, "kd_bn_nhwc_fwd: pixel stride below C");
    KD_REQUIRE(training || (running_mean && running_var), KD_ERR_INVALID, "kd_bn_nhwc_fwd: eval mode needs the running statistics");
    hipStream_t s = (hipStream_t)stream;
    if (training) {
        KD_REQUIRE(workspace && workspace_bytes >= kd_bn_nhwc_workspace(M, C), KD_ERR_WORKSPACE, "kd_bn_nhwc_fwd: workspace too small");
        launch_batch_stats(g, x, ldx, (float *)workspace, save_mean, save_invstd, running_mean, running_var, nullptr, momentum, eps, s);
        KD_CHECK_LAUNCH("kd_bn_nhwc_fwd(stats)");
    } else {
        hipLaunchKernelGGL(bn_nhwc_eval_stats_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, (int)C, (const float *)running_mean,
                           (const float *)running_var, eps, save_mean, save_invstd);
        KD_CHECK_LAUNCH("kd_bn_nhwc_fwd(eval)");
    }
    launch_apply(g, x, ldx, y, ldy, gamma, beta, save_mean, save_invstd, (int)relu, s);
    KD_CHECK_LAUNCH("kd_bn_nhwc_fwd(apply)");
    return KD_OK;
}

extern "C" int kd_bn_nhwc_bwd(const float *gy, int32_t ldg, const float *x, int32_t ldx, const float *y, int32_t ldy,
                              const float *res, int32_t ldres, float *dx, int32_t lddx, int64_t M, int32_t C, const float *gamma,
                              const float *save_mean, const float *save_invstd, float *dgamma, float *dbeta, int32_t accumulate,
                              int32_t training, int32_t relu, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    BnGeom g;
    if (int rc = geom(M, C, g, "kd_bn_nhwc_bwd")) return rc;
    KD_REQUIRE(gy && x && gamma && save_mean && save_invstd, KD_ERR_INVALID, "kd_bn_nhwc_bwd: null argument");
    KD_REQUIRE(!relu || y, KD_ERR_INVALID, "kd_bn_nhwc_bwd: the fused-ReLU backward needs the forward output");
    KD_REQUIRE(dx || dgamma || dbeta, KD_ERR_INVALID, "kd_bn_nhwc_bwd: nothing requested");
    KD_REQUIRE(ldg >= C && ldx >= C && (!y || ldy >= C) && (!res || ldres >= C) && (!dx || lddx >= C), KD_ERR_INVALID,
               "kd_bn_nhwc_bwd: pixel stride below C");
    hipStream_t s = (hipStream_t)stream;
    const bool need_sums = (dx && training) || dgamma || dbeta;
    float *sums = nullptr;
    if (need_sums) {
        KD_REQUIRE(workspace && workspace_bytes >= kd_bn_nhwc_workspace(M, C), KD_ERR_WORKSPACE, "kd_bn_nhwc_bwd: workspace too small");
        float *part = (float *)workspace;
        sums = part + (size_t)g.nrb * 3 * C;
        hipLaunchKernelGGL(bn_nhwc_grad_partial_kernel, dim3((unsigned)g.nrb, (unsigned)((C + 63) / 64)), dim3(TPB), 0, s, g, gy, ldg, x, ldx,
                           y, ldy, save_mean, save_invstd, (int)relu, part);
        KD_CHECK_LAUNCH("kd_bn_nhwc_bwd(partial)");
        hipLaunchKernelGGL(bn_nhwc_grad_finish_kernel, dim3((unsigned)((C + 63) / 64)), dim3(TPB), 0, s, g, (const float *)part, sums, dgamma,
                           dbeta, (int)accumulate);
        KD_CHECK_LAUNCH("kd_bn_nhwc_bwd(finish)");
    }
    if (!dx) {
        KD_NOTE_PLUMBING("bn_nhwc_grad_finish_kernel");
        return KD_OK;
    }
    if (vec4_ok(C, {{gy, ldg}, {x, ldx}, {relu ? y : nullptr, ldy}, {res, ldres}, {dx, lddx}})) {
        KD_NOTE_PLUMBING("bn_nhwc_dx_kernel<4>");
        hipLaunchKernelGGL(bn_nhwc_dx_kernel<4>, dim3(grid_for(M * (C / 4))), dim3(TPB), 0, s, g, gy, ldg, x, ldx, y, ldy, res, ldres, dx,
                           lddx, gamma, save_mean, save_invstd, (const float *)sums, (int)(training != 0), (int)relu);
    } else {
        KD_NOTE_PLUMBING("bn_nhwc_dx_kernel<1>");
        hipLaunchKernelGGL(bn_nhwc_dx_kernel<1>, dim3(grid_for(M * C)), dim3(TPB), 0, s, g, gy, ldg, x, ldx, y, ldy, res, ldres, dx, lddx,
                           gamma, save_mean, save_invstd, (const float *)sums, (int)(training != 0), (int)relu);
    }
    KD_CHECK_LAUNCH("kd_bn_nhwc_bwd(dx)");
    return KD_OK;
}
