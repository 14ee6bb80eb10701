// The NHWC BatchNorm, once, for both storages: the kernels (templated on the storage type T = float | bf16_t and on V, the
// channels a lane owns) and one implementation each of forward, backward, statistics-only and apply-only, which bn_nhwc.hip
// (kd_bn_nhwc_fwd / _bwd, kd_bn_nhwc_lp_fwd / _bwd) and dense_ops.hip (kd_bn_nhwc_stats / _apply) wrap.  Both files compile the
// same kernels, so statistics of a channel are the same bits whichever entry point computed them.
//
// x / y / gy / res / dx are T, widened to fp32 on load; every per-channel vector (gamma, beta, the saved and running statistics,
// dgamma, dbeta) is fp32; bf16 y and dx are rounded to nearest-even once, at the store.
//
// Every reduction is two fixed-order stages and no atomics, so results are bit-reproducible run to run:
//   stage 1 (one workgroup per ROWS pixels x 64 channels): per-block partials; in the forward the block sums x - k and
//           (x - k)^2 around k = the block's first pixel, so the fp32 sums see values of the order of the spread, not of the
//           mean (no E[x^2] - E[x]^2 cancellation when |mean| >> std);
//   stage 2: row-interleaved fp64 chains merged in a fixed order -- forward: 16 channels x 16 chains per workgroup, Chan's
//           pairwise update for mean / M2 and a fixed tree over the chains; backward: 64 channels x 4 chains, plain sums.
// A stage-1 workgroup is 256 threads = CL channel lanes x RL row lanes:
//   scalar (V = 1): 64 lanes of one channel x 4 row lanes -- a row lane is a wave;
//   vector (bf16, V = 8): 8 lanes of 8 channels (one 16-B load) x 32 row lanes, 8 of them in a wave.
// A thread keeps its sums in registers; the row lanes of a wave are folded with xor-shuffles (offsets 32 .. CL: a fixed tree, none
// for V = 1), and only the four wave totals go through LDS (2 KiB), added as (w0 + w1) + (w2 + w3).
// The elementwise pass is a separate grid-stride kernel: y = relu?((x - mean) * gamma * invstd + beta), resp. dx, 16 B a lane
// (V = 4 fp32 / 8 bf16) where the views allow it.
// Which variant runs, and on what grids, is bn_select.h's decision; the implementations below only check and launch.
#pragma once
#include "bn_select.h"
#include "kd_common.h"

namespace {

constexpr int ROWS = BN_ROWS;   // pixels per stage-1 workgroup
constexpr int TPB = BN_TPB;     // 64 channels x 4 row lanes
constexpr int FCH = BN_FWD_FINISH_CH, FL = TPB / FCH;
static_assert(TPB / 4 == BN_CBLOCK && BN_BWD_FINISH_CH == 64 && BN_VEC_BYTES == sizeof(float4), "bn_select.h plans the grids for this blocking");

template <typename T> constexpr int BN_V = BN_VEC_BYTES / (int)sizeof(T);        // elementwise vector width: 4 fp32, 8 bf16
template <typename T> constexpr int BN_PART_V = sizeof(T) == 2 ? BN_V<T> : 1;     // stage-1 vector width: the fp32 partials stay scalar

struct BnGeom {
    long long M;            // pixels (N*H*W)
    int C;
    int nrb;                // stage-1 row blocks = ceil(M / ROWS)
};

template <int V, typename T> __device__ __forceinline__ void ldv(const T *p, float (&v)[V])
{
    if constexpr (V == 8) {
        ld8(p, v);
    } else if constexpr (V == 4) {
        const float4 a = *(const float4 *)p;
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
        v[0] = Elem<T>::ld(p);
    }
}
template <int V, typename T> __device__ __forceinline__ void stv(T *p, const float (&v)[V])
{
    if constexpr (V == 8) st8(p, v);
    else if constexpr (V == 4) *(float4 *)p = make_float4(v[0], v[1], v[2], v[3]);
    else Elem<T>::st(p, v[0]);
}

// Folds s[q][j] over the row lanes of the workgroup: afterwards thread t < 64 returns in out[q] the total of channel t of the
// block (V * channel lane + j).  Every thread of the workgroup calls it.
template <int V, int NQ>
__device__ __forceinline__ void fold_row_lanes(float (&s)[NQ][V], float (&sh)[NQ][4][64], float (&out)[NQ])
{
    constexpr int CL = 64 / V;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tx = threadIdx.x % CL;
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float v = s[q][j];
#pragma unroll
            for (int o = 32; o >= CL; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane < CL) sh[q][wave][tx * V + j] = v;
        }
    __syncthreads();
    if (threadIdx.x < 64)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            out[q] = (sh[q][0][threadIdx.x] + sh[q][1][threadIdx.x]) + (sh[q][2][threadIdx.x] + sh[q][3][threadIdx.x]);
}

// stage 1 forward: part[rb][0][c] = k, part[rb][1][c] = sum (x - k), part[rb][2][c] = sum (x - k)^2 over the block's pixels
template <typename T, int V>
__global__ __launch_bounds__(TPB) void bn_nhwc_stats_partial_kernel(BnGeom g, const T *__restrict__ x, int ldx, float *__restrict__ part)
{
    constexpr int CL = 64 / V, RL = TPB / CL;
    __shared__ float sh[2][4][64];
    __shared__ float shk[64];
    const int tx = threadIdx.x % CL, ty = threadIdx.x / CL;
    const int c0 = blockIdx.y * 64 + tx * V, rb = blockIdx.x;
    const long long r0 = (long long)rb * ROWS;
    const long long r1 = r0 + ROWS < g.M ? r0 + ROWS : g.M;
    float s[2][V] = {};
    if (c0 < g.C) {
        float k[V];
        ldv<V>(x + r0 * ldx + c0, k);
        for (long long r = r0 + ty; r < r1; r += RL) {
            float v[V];
            ldv<V>(x + r * ldx + c0, v);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float d = v[j] - k[j];
                s[0][j] += d;
                s[1][j] = fmaf(d, d, s[1][j]);
            }
        }
        if (ty == 0)
#pragma unroll
            for (int j = 0; j < V; ++j) shk[tx * V + j] = k[j];
    }
    float tot[2];
    fold_row_lanes<V, 2>(s, sh, tot);
    const int c = blockIdx.y * 64 + threadIdx.x;
    if (threadIdx.x < 64 && c < g.C) {
        float *p = part + (size_t)rb * 3 * g.C;
        p[c] = shk[threadIdx.x];
        p[g.C + c] = tot[0];
        p[2 * g.C + c] = tot[1];
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

// y[m][c] = T(relu?((x - mean) * (gamma * invstd) + beta)), V channels per thread
template <typename T, int V>
__global__ __launch_bounds__(TPB) void bn_nhwc_apply_kernel(BnGeom g, const T *__restrict__ x, int ldx, T *__restrict__ y, int ldy,
                                                            const float *__restrict__ gamma, const float *__restrict__ beta,
                                                            const float *__restrict__ mean, const float *__restrict__ invstd, int relu)
{
    const int cv = g.C / V;
    const long long total = g.M * cv;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const long long m = i / cv;
        const int c0 = (int)(i - m * cv) * V;
        float v[V];
        ldv<V>(x + m * ldx + c0, v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int c = c0 + j;
            const float o = fmaf(v[j] - mean[c], gamma[c] * invstd[c], beta[c]);
            v[j] = relu ? fmaxf(o, 0.f) : o;
        }
        stv<V>(y + m * ldy + c0, v);
    }
}

// stage 1 backward: part[rb][0][c] = sum g', part[rb][1][c] = sum g' * xhat (g' = relu ? g * [y > 0] : g, y as stored)
template <typename T, int V>
__global__ __launch_bounds__(TPB) void bn_nhwc_grad_partial_kernel(BnGeom g, const T *__restrict__ gy, int ldg, const T *__restrict__ x, int ldx,
                                                                   const T *__restrict__ y, int ldy, const float *__restrict__ mean,
                                                                   const float *__restrict__ invstd, int relu, float *__restrict__ part)
{
    constexpr int CL = 64 / V, RL = TPB / CL;
    __shared__ float sh[2][4][64];
    const int tx = threadIdx.x % CL, ty = threadIdx.x / CL;
    const int c0 = blockIdx.y * 64 + tx * V, rb = blockIdx.x;
    const long long r0 = (long long)rb * ROWS;
    const long long r1 = r0 + ROWS < g.M ? r0 + ROWS : g.M;
    float s[2][V] = {};
    if (c0 < g.C) {
        float mu[V], is[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            mu[j] = mean[c0 + j];
            is[j] = invstd[c0 + j];
        }
        for (long long r = r0 + ty; r < r1; r += RL) {
            float gv[V], xv[V], yv[V];
            ldv<V>(gy + r * ldg + c0, gv);
            ldv<V>(x + r * ldx + c0, xv);
            if (relu) ldv<V>(y + r * ldy + c0, yv);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float t = (relu && !(yv[j] > 0.f)) ? 0.f : gv[j];
                s[0][j] += t;
                s[1][j] = fmaf(t, (xv[j] - mu[j]) * is[j], s[1][j]);
            }
        }
    }
    float tot[2];
    fold_row_lanes<V, 2>(s, sh, tot);
    const int c = blockIdx.y * 64 + threadIdx.x;
    if (threadIdx.x < 64 && c < g.C) {
        float *p = part + (size_t)rb * 2 * g.C;
        p[c] = tot[0];
        p[g.C + c] = tot[1];
    }
}

// stage 2 backward: sums[0][c] = sum g', sums[1][c] = sum g' * xhat (64 channels x 4 fp64 chains); dbeta / dgamma (+)= them when given
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

// dx = T(gamma * invstd * (g' - [training] (sum g' + xhat * sum g' xhat) / M) + res).  dx may be res itself: a thread loads
// its elements of res before it stores the same elements of dx and touches no others (so neither is __restrict__).
template <typename T, int V>
__global__ __launch_bounds__(TPB) void bn_nhwc_dx_kernel(BnGeom g, const T *__restrict__ gy, int ldg, const T *__restrict__ x, int ldx,
                                                         const T *__restrict__ y, int ldy, const T *res, int ldres, T *dx, int lddx,
                                                         const float *__restrict__ gamma, const float *__restrict__ mean,
                                                         const float *__restrict__ invstd, const float *__restrict__ sums, int training, int relu)
{
    const int cv = g.C / V;
    const long long total = g.M * cv;
    const float inv_m = (float)(1.0 / (double)g.M);
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const long long m = i / cv;
        const int c0 = (int)(i - m * cv) * V;
        float gv[V], xv[V], yv[V], rv[V], o[V];
        ldv<V>(gy + m * ldg + c0, gv);
        if (training) ldv<V>(x + m * ldx + c0, xv);
        if (relu) ldv<V>(y + m * ldy + c0, yv);
        if (res) ldv<V>(res + m * ldres + c0, rv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int c = c0 + j;
            const float is = invstd[c];
            float t = (relu && !(yv[j] > 0.f)) ? 0.f : gv[j];
            if (training) t = t - sums[c] * inv_m - (xv[j] - mean[c]) * is * (sums[g.C + c] * inv_m);
            o[j] = gamma[c] * is * t;
            if (res) o[j] += rv[j];
        }
        stv<V>(dx + m * lddx + c0, o);
    }
}

int geom(long long M, int C, BnGeom &g, const char *who)
{
    KD_REQUIRE(M > 0 && C > 0, KD_ERR_INVALID, "%s: bad shape M=%lld C=%d", who, M, C);
    KD_REQUIRE(M < (1ll << 31) && (M + ROWS - 1) / ROWS < 65536, KD_ERR_UNSUPPORTED, "%s: M=%lld exceeds the supported pixel count", who, M);
    KD_REQUIRE((C + 63) / 64 < 65536, KD_ERR_UNSUPPORTED, "%s: C=%d too large", who, C);
    g.M = M; g.C = C; g.nrb = bn_row_blocks(M);
    return KD_OK;
}

// The two statistics launches of a train-mode forward (workspace: bn_workspace(M, C) bytes): what kd_bn_nhwc_stats is.
template <typename T>
int bn_stats(const char *who, const BnSel &sel, const BnGeom &g, const T *x, int ldx, float *mean, float *invstd, float *run_mean, float *run_var,
             float *var_unb, float momentum, float eps, void *workspace, size_t workspace_bytes, hipStream_t s)
{
    KD_REQUIRE(workspace && workspace_bytes >= bn_workspace(g.M, g.C), KD_ERR_WORKSPACE, "%s: workspace too small", who);
    float *part = (float *)workspace;
    const auto partial = sel.part_vec ? bn_nhwc_stats_partial_kernel<T, BN_PART_V<T>> : bn_nhwc_stats_partial_kernel<T, 1>;
    hipLaunchKernelGGL(partial, dim3(sel.part_x, sel.part_y), dim3(TPB), 0, s, g, x, ldx, part);
    hipLaunchKernelGGL(bn_nhwc_stats_finish_kernel, dim3(sel.finish), dim3(TPB), 0, s, g, (const float *)part, mean, invstd, run_mean, run_var,
                       var_unb, momentum, eps);
    KD_CHECK_LAUNCHF("%s(stats)", who);
    return KD_OK;
}

// The elementwise normalise (+ ReLU) pass with given statistics: what kd_bn_nhwc_apply is behind its running-statistics update.
template <typename T>
int bn_apply(const char *who, const BnSel &sel, const BnGeom &g, const T *x, int ldx, T *y, int ldy, const float *gamma, const float *beta,
             const float *mean, const float *invstd, int relu, hipStream_t s)
{
    const auto apply = sel.vec ? bn_nhwc_apply_kernel<T, BN_V<T>> : bn_nhwc_apply_kernel<T, 1>;
    hipLaunchKernelGGL(apply, dim3(sel.grid), dim3(TPB), 0, s, g, x, ldx, y, ldy, gamma, beta, mean, invstd, relu);
    KD_CHECK_LAUNCHF("%s(apply)", who);
    return KD_OK;
}

template <typename T>
int bn_forward(const char *who, const T *x, int ldx, T *y, int ldy, long long M, int C, const float *gamma, const float *beta, float *save_mean,
               float *save_invstd, float *running_mean, float *running_var, float momentum, float eps, int training, int relu, void *workspace,
               size_t workspace_bytes, hipStream_t s)
{
    BnGeom g;
    if (int rc = geom(M, C, g, who)) return rc;
    KD_REQUIRE(x && y && gamma && beta && save_mean && save_invstd, KD_ERR_INVALID, "%s: null argument", who);
    KD_REQUIRE(ldx >= C && ldy >= C, KD_ERR_INVALID, "%s: pixel stride below C", who);
    KD_REQUIRE(training || (running_mean && running_var), KD_ERR_INVALID, "%s: eval mode needs the running statistics", who);
    const BnSel sel = bn_select_fwd((int)sizeof(T), x, ldx, y, ldy, M, C);
    if (training) {
        if (int rc = bn_stats(who, sel, g, x, ldx, save_mean, save_invstd, running_mean, running_var, nullptr, momentum, eps, workspace,
                              workspace_bytes, s))
            return rc;
    } else {
        hipLaunchKernelGGL(bn_nhwc_eval_stats_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, C, (const float *)running_mean,
                           (const float *)running_var, eps, save_mean, save_invstd);
        KD_CHECK_LAUNCHF("%s(eval)", who);
    }
    KD_NOTE_PLUMBING(bn_kernel_name(sel.kernel));
    return bn_apply(who, sel, g, x, ldx, y, ldy, gamma, beta, (const float *)save_mean, (const float *)save_invstd, relu, s);
}

template <typename T>
int bn_backward(const char *who, const T *gy, int ldg, const T *x, int ldx, const T *y, int ldy, const T *res, int ldres, T *dx, int lddx,
                long long M, int C, const float *gamma, const float *save_mean, const float *save_invstd, float *dgamma, float *dbeta,
                int accumulate, int training, int relu, void *workspace, size_t workspace_bytes, hipStream_t s)
{
    BnGeom g;
    if (int rc = geom(M, C, g, who)) return rc;
    KD_REQUIRE(gy && x && gamma && save_mean && save_invstd, KD_ERR_INVALID, "%s: null argument", who);
    KD_REQUIRE(!relu || y, KD_ERR_INVALID, "%s: the fused-ReLU backward needs the forward output", who);
    KD_REQUIRE(dx || dgamma || dbeta, KD_ERR_INVALID, "%s: nothing requested", who);
    KD_REQUIRE(ldg >= C && ldx >= C && (!y || ldy >= C) && (!res || ldres >= C) && (!dx || lddx >= C), KD_ERR_INVALID, "%s: pixel stride below C",
               who);
    if (!relu) y = nullptr;     // not read: out of the selection and the kernels, after the checks on the operands as passed
    if (!dx) res = nullptr;
    const bool need_sums = (dx && training) || dgamma || dbeta;
    KD_REQUIRE(!need_sums || (workspace && workspace_bytes >= bn_workspace(M, C)), KD_ERR_WORKSPACE, "%s: workspace too small", who);
    const BnSel sel = bn_select_bwd((int)sizeof(T), gy, ldg, x, ldx, y, ldy, res, ldres, dx, lddx, M, C);
    KD_NOTE_PLUMBING(bn_kernel_name(sel.kernel));
    float *sums = nullptr;
    if (need_sums) {
        float *part = (float *)workspace;
        sums = part + bn_sums_offset(M, C);
        const auto partial = sel.part_vec ? bn_nhwc_grad_partial_kernel<T, BN_PART_V<T>> : bn_nhwc_grad_partial_kernel<T, 1>;
        hipLaunchKernelGGL(partial, dim3(sel.part_x, sel.part_y), dim3(TPB), 0, s, g, gy, ldg, x, ldx, y, ldy, save_mean, save_invstd, relu, part);
        KD_CHECK_LAUNCHF("%s(partial)", who);
        hipLaunchKernelGGL(bn_nhwc_grad_finish_kernel, dim3(sel.finish), dim3(TPB), 0, s, g, (const float *)part, sums, dgamma, dbeta, accumulate);
        KD_CHECK_LAUNCHF("%s(finish)", who);
    }
    if (!dx) return KD_OK;
    const auto dxk = sel.vec ? bn_nhwc_dx_kernel<T, BN_V<T>> : bn_nhwc_dx_kernel<T, 1>;
    hipLaunchKernelGGL(dxk, dim3(sel.grid), dim3(TPB), 0, s, g, gy, ldg, x, ldx, y, ldy, res, ldres, dx, lddx, gamma, save_mean, save_invstd,
                       (const float *)sums, (int)(training != 0), relu);
    KD_CHECK_LAUNCHF("%s(dx)", who);
    return KD_OK;
}

}  // namespace
