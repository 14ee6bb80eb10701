// The classifier head of the CIFAR pre-activation ResNet (models/cifar_models/preresnet.py): BatchNorm -> ReLU -> average pool over
// the whole map, as one pass over x that never stores the activation (kd_head_bn_relu_pool_fwd), and its backward, which recomputes
// the activation's sign from x (kd_head_bn_relu_pool_bwd).
//
// A workgroup owns HEAD_GROUP = 4 consecutive channels over all N * HW pixels and needs nobody else's sums: no workspace, no atomics,
// and every sum is taken in a fixed order (a thread's pixels in ascending order, then a fixed tree), so the bits repeat from run to
// run.  A thread loads V = 4 channels of a pixel with one 16-B access or V = 1 with a scalar one; a workgroup is 4 / V channel lanes
// (fastest) x pixel lanes, 1024 threads: the walk over the pixels is strided (16 B of every pixel's row), so latency is hidden by
// waves, not by bandwidth.  Workgroups are dealt so that neighbouring channel groups, which share cache lines, share an XCD's L2
// (xcd_remap).  Forward: a wave takes the images n = wave, wave + 16, ..., its pixel lanes stride over the image's HW pixels
// and the wave's partial sums are folded with __shfl_xor.  Backward: the pixel lanes stride over all N * HW pixels for sum g' and
// sum g' xhat (g' = gpooled / HW where the activation is positive, 0 elsewhere), a tree in LDS folds them, and a second walk over
// the same pixels (from cache at CIFAR's sizes) writes dx.  Which instantiation runs is head_select.h's decision.
#include "head_select.h"
#include "kd_common.h"

namespace {

constexpr int TPB = HEAD_TPB, GROUP = HEAD_GROUP;
static_assert(TPB % 64 == 0 && 64 % GROUP == 0 && GROUP * sizeof(float) == HEAD_VEC_BYTES, "a channel group is one 16-B access");

template <int V> __device__ __forceinline__ void ldv(const float *p, float (&v)[V])
{
    if constexpr (V == 4) {
        const float4 a = *(const float4 *)p;
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = p[j];
    }
}
template <int V> __device__ __forceinline__ void stv(float *p, const float (&v)[V])
{
    if constexpr (V == 4) *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]);
    else {
#pragma unroll
        for (int j = 0; j < V; ++j) p[j] = v[j];
    }
}

// The BN operands of a thread's V channels (zeros for a channel lane past C: it loads and stores nothing, but takes part in the folds).
template <int V> struct Chan {
    float g[V], b[V], mu[V], is[V];
    __device__ __forceinline__ Chan(bool live, int c0, const float *gamma, const float *beta, const float *mean, const float *invstd)
    {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            g[j] = live ? gamma[c0 + j] : 0.f;
            b[j] = live ? beta[c0 + j] : 0.f;
            mu[j] = live ? mean[c0 + j] : 0.f;
            is[j] = live ? invstd[c0 + j] : 0.f;
        }
    }
};

// running <- (1 - momentum) running + momentum v, the expression of the NHWC BatchNorm kernels
__device__ __forceinline__ float running_update(float running, float momentum, float v) { return (1.f - momentum) * running + momentum * v; }

template <int V>
__global__ __launch_bounds__(TPB) void head_fwd_kernel(const float *__restrict__ x, int ldx, int N, int HW, int C, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, const float *__restrict__ mean,
                                                       const float *__restrict__ invstd, float *__restrict__ pooled,
                                                       const float *__restrict__ var_unb, float *__restrict__ run_mean,
                                                       float *__restrict__ run_var, float momentum)
{
    constexpr int CL = GROUP / V, PLW = 64 / CL;          // channel lanes; pixel lanes of a wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cl = lane % CL, pl = lane / CL;
    const int c0 = xcd_remap(blockIdx.x, gridDim.x) * GROUP + cl * V;     // (V == 4: C % 4 == 0, every lane is live)
    const bool live = c0 < C;
    const Chan<V> ch(live, c0, gamma, beta, mean, invstd);
    if (wave == 0 && pl == 0 && live) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (run_mean) run_mean[c0 + j] = running_update(run_mean[c0 + j], momentum, ch.mu[j]);
            if (run_var) run_var[c0 + j] = running_update(run_var[c0 + j], momentum, var_unb[c0 + j]);
        }
    }
    const float hw = (float)HW;
    for (int n = wave; n < N; n += TPB / 64) {
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.f;
        if (live) {
            const float *xn = x + (long long)n * HW * ldx + c0;
            for (int p = pl; p < HW; p += PLW) {
                float v[V];
                ldv<V>(xn + (long long)p * ldx, v);
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float y = (v[j] - ch.mu[j]) * ch.is[j] * ch.g[j] + ch.b[j];
                    acc[j] += y < 0.f ? 0.f : y;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < V; ++j)
#pragma unroll
            for (int o = 32; o >= CL; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
        if (live && pl == 0) {
#pragma unroll
            for (int j = 0; j < V; ++j) pooled[(long long)n * C + c0 + j] = acc[j] / hw;
        }
    }
}

template <int V>
__global__ __launch_bounds__(TPB) void head_bwd_kernel(const float *__restrict__ x, int ldx, const float *__restrict__ gpooled, int N, int HW, int C,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       const float *__restrict__ mean, const float *__restrict__ invstd, float *__restrict__ dx,
                                                       int lddx, float *__restrict__ dgamma, float *__restrict__ dbeta, int training)
{
    constexpr int CL = GROUP / V, PL = TPB / CL;          // channel lanes; pixel lanes of the workgroup
    __shared__ float red[2][GROUP][PL];
    const int cl = threadIdx.x % CL, pl = threadIdx.x / CL;
    const int c0 = xcd_remap(blockIdx.x, gridDim.x) * GROUP + cl * V;
    const bool live = c0 < C;
    const Chan<V> ch(live, c0, gamma, beta, mean, invstd);
    const long long M = (long long)N * HW;
    const float hw = (float)HW;
    float sg[V], sb[V];
#pragma unroll
    for (int j = 0; j < V; ++j) sg[j] = sb[j] = 0.f;
    if (live) {
        for (long long m = pl; m < M; m += PL) {
            const float *gp = gpooled + (m / HW) * C + c0;
            float v[V];
            ldv<V>(x + m * ldx + c0, v);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float xh = (v[j] - ch.mu[j]) * ch.is[j];
                const float y = xh * ch.g[j] + ch.b[j];
                const float gy = y > 0.f ? gp[j] / hw : 0.f;
                sb[j] += gy;
                sg[j] += gy * xh;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        red[0][cl * V + j][pl] = sg[j];
        red[1][cl * V + j][pl] = sb[j];
    }
    __syncthreads();
    for (int s = PL / 2; s > 0; s >>= 1) {
        if (pl < s) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                red[0][cl * V + j][pl] += red[0][cl * V + j][pl + s];
                red[1][cl * V + j][pl] += red[1][cl * V + j][pl + s];
            }
        }
        __syncthreads();
    }
    if (!live) return;                                    // (no barrier below)
#pragma unroll
    for (int j = 0; j < V; ++j) {
        sg[j] = red[0][cl * V + j][0];
        sb[j] = red[1][cl * V + j][0];
    }
    if (pl == 0) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            dgamma[c0 + j] = sg[j];
            dbeta[c0 + j] = sb[j];
        }
    }
    if (!dx) return;
    const float fm = (float)M;
    float mg[V], mb[V], k[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        mg[j] = training ? sg[j] / fm : 0.f;
        mb[j] = training ? sb[j] / fm : 0.f;
        k[j] = ch.g[j] * ch.is[j];
    }
    for (long long m = pl; m < M; m += PL) {
        const float *gp = gpooled + (m / HW) * C + c0;
        float v[V], d[V];
        ldv<V>(x + m * ldx + c0, v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float xh = (v[j] - ch.mu[j]) * ch.is[j];
            const float y = xh * ch.g[j] + ch.b[j];
            const float gy = y > 0.f ? gp[j] / hw : 0.f;
            d[j] = k[j] * (gy - mb[j] - xh * mg[j]);
        }
        stv<V>(dx + m * lddx + c0, d);
    }
}

bool aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

extern "C" int kd_head_bn_relu_pool_fwd(const float *x, int32_t ldx, int32_t N, int32_t HW, int32_t C, const float *gamma, const float *beta,
                                        const float *mean, const float *invstd, float *pooled, const float *var_unbiased, float *running_mean,
                                        float *running_var, float momentum, kd_stream_t stream)
{
    KD_REQUIRE(x && gamma && beta && mean && invstd && pooled, KD_ERR_INVALID, "kd_head_bn_relu_pool_fwd: null argument");
    KD_REQUIRE(head_shape_ok(N, HW, C, ldx), KD_ERR_INVALID, "kd_head_bn_relu_pool_fwd: N = %d, HW = %d, C = %d, pixel stride %d", (int)N, (int)HW,
               (int)C, (int)ldx);
    KD_REQUIRE(!running_var || var_unbiased, KD_ERR_INVALID, "kd_head_bn_relu_pool_fwd: running_var without var_unbiased");
    KD_REQUIRE(aligned4(x) && aligned4(gamma) && aligned4(beta) && aligned4(mean) && aligned4(invstd) && aligned4(pooled) && aligned4(var_unbiased) &&
                   aligned4(running_mean) && aligned4(running_var),
               KD_ERR_INVALID, "kd_head_bn_relu_pool_fwd: an operand is not aligned to its element");
    const HeadSel sel = head_select(false, C, x, ldx, nullptr, 0);
    KD_NOTE_PLUMBING(head_kernel_name(sel.kernel));
    const dim3 grid(sel.grid), block(TPB);
    hipStream_t s = (hipStream_t)stream;
    if (sel.vec == 1)
        hipLaunchKernelGGL(head_fwd_kernel<1>, grid, block, 0, s, x, ldx, N, HW, C, gamma, beta, mean, invstd, pooled, var_unbiased, running_mean,
                           running_var, momentum);
    else
        hipLaunchKernelGGL(head_fwd_kernel<GROUP>, grid, block, 0, s, x, ldx, N, HW, C, gamma, beta, mean, invstd, pooled, var_unbiased, running_mean,
                           running_var, momentum);
    KD_CHECK_LAUNCH("kd_head_bn_relu_pool_fwd");
    return KD_OK;
}

extern "C" int kd_head_bn_relu_pool_bwd(const float *x, int32_t ldx, const float *gpooled, int32_t N, int32_t HW, int32_t C, const float *gamma,
                                        const float *beta, const float *mean, const float *invstd, float *dx, int32_t lddx, float *dgamma,
                                        float *dbeta, int32_t training, kd_stream_t stream)
{
    KD_REQUIRE(x && gpooled && gamma && beta && mean && invstd && dgamma && dbeta, KD_ERR_INVALID, "kd_head_bn_relu_pool_bwd: null argument");
    KD_REQUIRE(head_shape_ok(N, HW, C, ldx), KD_ERR_INVALID, "kd_head_bn_relu_pool_bwd: N = %d, HW = %d, C = %d, pixel stride %d", (int)N, (int)HW,
               (int)C, (int)ldx);
    KD_REQUIRE(!dx || lddx >= C, KD_ERR_INVALID, "kd_head_bn_relu_pool_bwd: dx pixel stride %d below C = %d", (int)lddx, (int)C);
    KD_REQUIRE(aligned4(x) && aligned4(gpooled) && aligned4(gamma) && aligned4(beta) && aligned4(mean) && aligned4(invstd) && aligned4(dx) &&
                   aligned4(dgamma) && aligned4(dbeta),
               KD_ERR_INVALID, "kd_head_bn_relu_pool_bwd: an operand is not aligned to its element");
    const HeadSel sel = head_select(true, C, x, ldx, dx, lddx);
    KD_NOTE_PLUMBING(head_kernel_name(sel.kernel));
    const dim3 grid(sel.grid), block(TPB);
    hipStream_t s = (hipStream_t)stream;
    const int tr = training != 0;
    if (sel.vec == 1)
        hipLaunchKernelGGL(head_bwd_kernel<1>, grid, block, 0, s, x, ldx, gpooled, N, HW, C, gamma, beta, mean, invstd, dx, lddx, dgamma, dbeta, tr);
    else
        hipLaunchKernelGGL(head_bwd_kernel<GROUP>, grid, block, 0, s, x, ldx, gpooled, N, HW, C, gamma, beta, mean, invstd, dx, lddx, dgamma, dbeta, tr);
    KD_CHECK_LAUNCH("kd_head_bn_relu_pool_bwd");
    return KD_OK;
}
