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

// stage 2 forward: batch mean / biased variance per channel; save_mean / save_invstd; running statistics (unbiased variance).
// A workgroup takes FCH channels with FL row-interleaved fp64 chains each (chain l merges row blocks l, l + FL, ...), then the
// FL chains are merged by a fixed pairwise tree (chain l takes in chain l + 8, then l + 4, l + 2, l + 1): ceil(C / 16) workgroups.
constexpr int FCH = 16, FL = TPB / FCH;
__global__ __launch_bounds__(TPB) void bn_nhwc_stats_finish_kernel(BnGeom g, const float *__restrict__ part,
                                                                   float *__restrict__ save_mean, float *__restrict__ save_invstd,
                                                                   float *__restrict__ run_mean, float *__restrict__ run_var,
                                                                   float momentum, float eps)
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
    if (run_mean) run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)mean;
    if (run_var) run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)(g.M > 1 ? m2 / (double)(g.M - 1) : var);
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

}  // namespace

extern "C" size_t kd_bn_nhwc_workspace(int64_t M, int32_t C)
{
    if (M <= 0 || C <= 0) return 0;
    const size_t nrb = (size_t)((M + ROWS - 1) / ROWS);
    return (nrb * 3 * (size_t)C + 2 * (size_t)C) * sizeof(float);
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
        float *part = (float *)workspace;
        hipLaunchKernelGGL(bn_nhwc_stats_partial_kernel, dim3((unsigned)g.nrb, (unsigned)((C + 63) / 64)), dim3(TPB), 0, s, g, x, ldx, part);
        KD_CHECK_LAUNCH("kd_bn_nhwc_fwd(partial)");
        hipLaunchKernelGGL(bn_nhwc_stats_finish_kernel, dim3((unsigned)((C + FCH - 1) / FCH)), dim3(TPB), 0, s, g, (const float *)part, save_mean,
                           save_invstd, running_mean, running_var, momentum, eps);
        KD_CHECK_LAUNCH("kd_bn_nhwc_fwd(finish)");
    } else {
        hipLaunchKernelGGL(bn_nhwc_eval_stats_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, (int)C, (const float *)running_mean,
                           (const float *)running_var, eps, save_mean, save_invstd);
        KD_CHECK_LAUNCH("kd_bn_nhwc_fwd(eval)");
    }
    if (vec4_ok(C, {{x, ldx}, {y, ldy}}))
        hipLaunchKernelGGL(bn_nhwc_apply_kernel<4>, dim3(grid_for(M * (C / 4))), dim3(TPB), 0, s, g, x, ldx, y, ldy, gamma, beta,
                           (const float *)save_mean, (const float *)save_invstd, (int)relu);
    else
        hipLaunchKernelGGL(bn_nhwc_apply_kernel<1>, dim3(grid_for(M * C)), dim3(TPB), 0, s, g, x, ldx, y, ldy, gamma, beta,
                           (const float *)save_mean, (const float *)save_invstd, (int)relu);
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
    if (!dx) return KD_OK;
    if (vec4_ok(C, {{gy, ldg}, {x, ldx}, {relu ? y : nullptr, ldy}, {res, ldres}, {dx, lddx}}))
        hipLaunchKernelGGL(bn_nhwc_dx_kernel<4>, dim3(grid_for(M * (C / 4))), dim3(TPB), 0, s, g, gy, ldg, x, ldx, y, ldy, res, ldres, dx,
                           lddx, gamma, save_mean, save_invstd, (const float *)sums, (int)(training != 0), (int)relu);
    else
        hipLaunchKernelGGL(bn_nhwc_dx_kernel<1>, dim3(grid_for(M * C)), dim3(TPB), 0, s, g, gy, ldg, x, ldx, y, ldy, res, ldres, dx, lddx,
                           gamma, save_mean, save_invstd, (const float *)sums, (int)(training != 0), (int)relu);
    KD_CHECK_LAUNCH("kd_bn_nhwc_bwd(dx)");
    return KD_OK;
}
