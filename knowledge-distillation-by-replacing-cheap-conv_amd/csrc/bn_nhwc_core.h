// Device code shared by bn_nhwc.hip (kd_bn_nhwc_fwd / _bwd) and dense_ops.hip (kd_bn_nhwc_stats / _apply): the two-stage
// fixed-order batch-statistics reduction (per-128-pixel shifted partials, fp64 Chan merge, no atomics), the elementwise
// normalise (+ ReLU) pass and the launch helpers.  Both files compile the same kernels, so statistics of a channel are the
// same bits whichever entry point computed them.
#pragma once
#include <initializer_list>
#include <utility>
#include "kd_common.h"

namespace {

constexpr int ROWS = 128;   // pixels per stage-1 workgroup
constexpr int TPB = 256;    // 64 channels x 4 row lanes

struct BnGeom {
    long long M;            // pixels (N*H*W)
    int C;
    int nrb;                // stage-1 row blocks = ceil(M / ROWS)
};

// stage 1 forward: part[rb][0][c] = k, part[rb][1][c] = sum (x - k), part[rb][2][c] = sum (x - k)^2 over the block's pixels
__global__ __launch_bounds__(TPB) void bn_nhwc_stats_partial_kernel(BnGeom g, const float *__restrict__ x, int ldx,
                                                                    float *__restrict__ part)
{
    __shared__ float sh[2][4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + tx, rb = blockIdx.x;
    const long long r0 = (long long)rb * ROWS;
    const long long r1 = r0 + ROWS < g.M ? r0 + ROWS : g.M;
    float k = 0.f, s1 = 0.f, s2 = 0.f;
    if (c < g.C) {
        k = x[r0 * ldx + c];
        for (long long r = r0 + ty; r < r1; r += 4) {
            const float v = x[r * ldx + c] - k;
            s1 += v;
            s2 = fmaf(v, v, s2);
        }
    }
    sh[0][ty][tx] = s1;
    sh[1][ty][tx] = s2;
    __syncthreads();
    if (ty == 0 && c < g.C) {
        float *p = part + (size_t)rb * 3 * g.C;
        p[c] = k;
        p[g.C + c] = (sh[0][0][tx] + sh[0][1][tx]) + (sh[0][2][tx] + sh[0][3][tx]);
        p[2 * g.C + c] = (sh[1][0][tx] + sh[1][1][tx]) + (sh[1][2][tx] + sh[1][3][tx]);
    }
}

// (n, mean, M2) += (nb, mb, M2b): Chan et al.'s pairwise update, fp64
__device__ __forceinline__ void chan_merge(double &n, double &mean, double &m2, double nb, double mb, double m2b)
{
    if (nb <= 0.0) return;
    const double t = n + nb, d = mb - mean;
    mean += d * (nb / t);
    m2 += m2b + d * d * (n * nb / t);
    n = t;
}

// running <- (1 - momentum) running + momentum v (v = the batch mean, resp. the unbiased batch variance, rounded to fp32)
__device__ __forceinline__ float bn_running_update(float running, float momentum, float v)
{
    return (1.f - momentum) * running + momentum * v;
}

// stage 2 forward: batch mean / biased variance per channel; save_mean / save_invstd; running statistics (unbiased variance,
// also stored to var_unb when given).
// A workgroup takes FCH channels with FL row-interleaved fp64 chains each (chain l merges row blocks l, l + FL, ...), then the
// FL chains are merged by a fixed pairwise tree (chain l takes in chain l + 8, then l + 4, l + 2, l + 1): ceil(C / 16) workgroups.
constexpr int FCH = 16, FL = TPB / FCH;
__global__ __launch_bounds__(TPB) void bn_nhwc_stats_finish_kernel(BnGeom g, const float *__restrict__ part,
                                                                   float *__restrict__ save_mean, float *__restrict__ save_invstd,
                                                                   float *__restrict__ run_mean, float *__restrict__ run_var,
                                                                   float *__restrict__ var_unb, float momentum, float eps)
{
    __shared__ double sh[3][FL][FCH];
    const int tx = threadIdx.x % FCH, ty = threadIdx.x / FCH;
    const int c = blockIdx.x * FCH + tx;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    if (c < g.C) {
        for (int rb = ty; rb < g.nrb; rb += FL) {
            const float *p = part + (size_t)rb * 3 * g.C;
            const long long r0 = (long long)rb * ROWS;
            const double nb = (double)((r0 + ROWS < g.M ? r0 + ROWS : g.M) - r0);
            const double s1 = p[g.C + c], s2 = p[2 * g.C + c];
            chan_merge(n, mean, m2, nb, (double)p[c] + s1 / nb, fmax(s2 - s1 * s1 / nb, 0.0));
        }
    }
    sh[0][ty][tx] = n;
    sh[1][ty][tx] = mean;
    sh[2][ty][tx] = m2;
    __syncthreads();
#pragma unroll
    for (int h = FL / 2; h > 0; h >>= 1) {
        if (ty < h) {
            chan_merge(n, mean, m2, sh[0][ty + h][tx], sh[1][ty + h][tx], sh[2][ty + h][tx]);
            sh[0][ty][tx] = n;
            sh[1][ty][tx] = mean;
            sh[2][ty][tx] = m2;
        }
        __syncthreads();
    }
    if (ty != 0 || c >= g.C) return;
    const double var = m2 / (double)g.M;
    save_mean[c] = (float)mean;
    save_invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    const float vu = (float)(g.M > 1 ? m2 / (double)(g.M - 1) : var);
    if (run_mean) run_mean[c] = bn_running_update(run_mean[c], momentum, (float)mean);
    if (run_var) run_var[c] = bn_running_update(run_var[c], momentum, vu);
    if (var_unb) var_unb[c] = vu;
}

__global__ void bn_nhwc_eval_stats_kernel(int C, const float *__restrict__ run_mean, const float *__restrict__ run_var, float eps,
                                          float *__restrict__ save_mean, float *__restrict__ save_invstd)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    save_mean[c] = run_mean[c];
    save_invstd[c] = (float)(1.0 / sqrt((double)run_var[c] + (double)eps));
}

// y[m][c] = relu?((x - mean) * (gamma * invstd) + beta), 4 channels per thread when C % 4 == 0 and the views allow float4
template <int V>
__global__ __launch_bounds__(TPB) void bn_nhwc_apply_kernel(BnGeom g, const float *__restrict__ x, int ldx, float *__restrict__ y,
                                                            int ldy, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                            const float *__restrict__ mean, const float *__restrict__ invstd, int relu)
{
    const int cv = g.C / V;
    const long long total = g.M * cv;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const long long m = i / cv;
        const int c0 = (int)(i - m * cv) * V;
        float v[V];
        if constexpr (V == 4) {
            const float4 a = *(const float4 *)(x + m * ldx + c0);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        } else {
            v[0] = x[m * ldx + c0];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int c = c0 + j;
            const float o = fmaf(v[j] - mean[c], gamma[c] * invstd[c], beta[c]);
            v[j] = relu ? fmaxf(o, 0.f) : o;
        }
        if constexpr (V == 4) *(float4 *)(y + m * ldy + c0) = make_float4(v[0], v[1], v[2], v[3]);
        else y[m * ldy + c0] = v[0];
    }
}

inline int grid_for(long long total)
{
    long long b = (total + TPB - 1) / TPB;
    return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

// float4 path: C % 4 == 0, every pixel stride % 4 == 0, every base 16-B aligned
inline bool vec4_ok(int C, std::initializer_list<std::pair<const float *, int>> views)
{
    if (C % 4) return false;
    for (auto &v : views)
        if (v.first && (v.second % 4 || !kd_aligned16(v.first))) return false;
    return true;
}

int geom(long long M, int C, BnGeom &g, const char *who)
{
    KD_REQUIRE(M > 0 && C > 0, KD_ERR_INVALID, "%s: bad shape M=%lld C=%d", who, M, C);
    KD_REQUIRE(M < (1ll << 31) && (M + ROWS - 1) / ROWS < 65536, KD_ERR_UNSUPPORTED, "%s: M=%lld exceeds the supported pixel count", who, M);
    KD_REQUIRE((C + 63) / 64 < 65536, KD_ERR_UNSUPPORTED, "%s: C=%d too large", who, C);
    g.M = M; g.C = C; g.nrb = (int)((M + ROWS - 1) / ROWS);
    return KD_OK;
}

// the two statistics launches of a train-mode forward (part: kd_bn_nhwc_workspace(M, C) bytes)
inline void launch_batch_stats(const BnGeom &g, const float *x, int ldx, float *part, float *save_mean, float *save_invstd, float *run_mean,
                               float *run_var, float *var_unb, float momentum, float eps, hipStream_t s)
{
    hipLaunchKernelGGL(bn_nhwc_stats_partial_kernel, dim3((unsigned)g.nrb, (unsigned)((g.C + 63) / 64)), dim3(TPB), 0, s, g, x, ldx, part);
    hipLaunchKernelGGL(bn_nhwc_stats_finish_kernel, dim3((unsigned)((g.C + FCH - 1) / FCH)), dim3(TPB), 0, s, g, (const float *)part, save_mean,
                       save_invstd, run_mean, run_var, var_unb, momentum, eps);
}

inline void launch_apply(const BnGeom &g, const float *x, int ldx, float *y, int ldy, const float *gamma, const float *beta,
                         const float *mean, const float *invstd, int relu, hipStream_t s)
{
    if (vec4_ok(g.C, {{x, ldx}, {y, ldy}})) {
        KD_NOTE_PLUMBING("bn_nhwc_apply_kernel<4>");
        hipLaunchKernelGGL(bn_nhwc_apply_kernel<4>, dim3(grid_for(g.M * (g.C / 4))), dim3(TPB), 0, s, g, x, ldx, y, ldy, gamma, beta, mean, invstd,
                           relu);
    } else {
        KD_NOTE_PLUMBING("bn_nhwc_apply_kernel<1>");
        hipLaunchKernelGGL(bn_nhwc_apply_kernel<1>, dim3(grid_for(g.M * g.C)), dim3(TPB), 0, s, g, x, ldx, y, ldy, gamma, beta, mean, invstd, relu);
    }
}

inline size_t bn_workspace_bytes(long long M, int C)
{
    if (M <= 0 || C <= 0) return 0;
    const size_t nrb = (size_t)((M + ROWS - 1) / ROWS);
    return (nrb * 3 * (size_t)C + 2 * (size_t)C) * sizeof(float);
}

}  // namespace
