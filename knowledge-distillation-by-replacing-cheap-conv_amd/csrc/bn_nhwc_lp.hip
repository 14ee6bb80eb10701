// BatchNorm2d on NHWC bf16 views: the bf16 twin of bn_nhwc.hip for the Wide-ResNet CIFAR path (kd_bn_nhwc_lp_fwd / _bwd).
// x / y / gy / res / dx are bf16 storage, widened to fp32 on load; every per-channel vector (gamma, beta, the saved and running
// statistics, dgamma, dbeta) stays fp32; y and dx are rounded to nearest-even once, at the store.
//
// The reductions are those of bn_nhwc_core.h: stage 1 takes per-128-pixel partials (the forward around k = the block's first
// pixel), stage 2 merges them in fp64 in a fixed order (the forward's finish IS bn_nhwc_stats_finish_kernel) -- no atomics, so two
// runs give the same bits.  A stage-1 workgroup owns 128 pixels x 64 channels as 256 threads = CL channel lanes x RL row lanes:
//   scalar (V = 1): 64 lanes of one channel x 4 row lanes -- a row lane is a wave, as in the fp32 kernels;
//   vector (V = 8): 8 lanes of 8 channels (one 16-B load) x 32 row lanes, 8 of them in a wave.
// A thread keeps its sums in registers; the row lanes of a wave are folded with xor-shuffles (offsets 32 .. CL: a fixed tree), and
// only the four wave totals go through LDS (2 KiB), not a [row lane][channel] table.
// Which variant runs, and on what grids, is bn_lp_select.h's decision; the launchers below only launch.
#include "bn_lp_select.h"
#include "bn_nhwc_core.h"

namespace {

static_assert(ROWS == BN_LP_ROWS && TPB == BN_LP_TPB && FCH == BN_LP_FWD_FINISH_CH && TPB / 4 == BN_LP_CBLOCK && BN_LP_BWD_FINISH_CH == 64,
              "bn_lp_select.h plans the grids for this blocking");

template <int V> __device__ __forceinline__ void ldv(const bf16_t *p, float (&v)[V])
{
    if constexpr (V == 8) ld8(p, v);
    else v[0] = bf16_to_f32(*p);
}
template <int V> __device__ __forceinline__ void stv(bf16_t *p, const float (&v)[V])
{
    if constexpr (V == 8) st8(p, v);
    else *p = f32_to_bf16(v[0]);
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

// stage 1 forward: part[rb][0][c] = k, part[rb][1][c] = sum (x - k), part[rb][2][c] = sum (x - k)^2 (bn_nhwc_stats_finish_kernel's input)
template <int V>
__global__ __launch_bounds__(TPB) void bn_lp_stats_partial_kernel(BnGeom g, const bf16_t *__restrict__ x, int ldx, float *__restrict__ part)
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

// stage 1 backward: part[rb][0][c] = sum g', part[rb][1][c] = sum g' * xhat (g' = relu ? g * [y > 0] : g, y the stored bf16)
template <int V>
__global__ __launch_bounds__(TPB) void bn_lp_grad_partial_kernel(BnGeom g, const bf16_t *__restrict__ gy, int ldg, const bf16_t *__restrict__ x,
                                                                 int ldx, const bf16_t *__restrict__ y, int ldy,
                                                                 const float *__restrict__ mean, const float *__restrict__ invstd, int relu,
                                                                 float *__restrict__ part)
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
__global__ __launch_bounds__(TPB) void bn_lp_grad_finish_kernel(BnGeom g, const float *__restrict__ part, float *__restrict__ sums,
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

// y[m][c] = bf16(relu?((x - mean) * (gamma * invstd) + beta)), V channels per thread
template <int V>
__global__ __launch_bounds__(TPB) void bn_lp_apply_kernel(BnGeom g, const bf16_t *__restrict__ x, int ldx, bf16_t *__restrict__ y, int ldy,
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

// dx = bf16(gamma * invstd * (g' - [training] (sum g' + xhat * sum g' xhat) / M) + res).  dx may be res itself: a thread loads
// its elements of res before it stores the same elements of dx and touches no others (so neither is __restrict__).
template <int V>
__global__ __launch_bounds__(TPB) void bn_lp_dx_kernel(BnGeom g, const bf16_t *__restrict__ gy, int ldg, const bf16_t *__restrict__ x, int ldx,
                                                       const bf16_t *__restrict__ y, int ldy, const bf16_t *res, int ldres, bf16_t *dx, int lddx,
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

template <int V>
void launch_lp_fwd_stats(const BnLpSel &sel, const BnGeom &g, const bf16_t *x, int ldx, float *part, float *save_mean, float *save_invstd,
                         float *run_mean, float *run_var, float momentum, float eps, hipStream_t s)
{
    hipLaunchKernelGGL(bn_lp_stats_partial_kernel<V>, dim3(sel.part_x, sel.part_y), dim3(TPB), 0, s, g, x, ldx, part);
    hipLaunchKernelGGL(bn_nhwc_stats_finish_kernel, dim3(sel.finish), dim3(TPB), 0, s, g, (const float *)part, save_mean, save_invstd, run_mean,
                       run_var, (float *)nullptr, momentum, eps);
}

}  // namespace

extern "C" size_t kd_bn_nhwc_lp_workspace(int64_t M, int32_t C)
{
    return bn_lp_workspace(M, C);
}

extern "C" int kd_bn_nhwc_lp_fwd(const void *x_, int32_t ldx, void *y_, int32_t ldy, int64_t M, int32_t C, const float *gamma, const float *beta,
                                 float *save_mean, float *save_invstd, float *running_mean, float *running_var, float momentum, float eps,
                                 int32_t training, int32_t relu, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    BnGeom g;
    if (int rc = geom(M, C, g, "kd_bn_nhwc_lp_fwd")) return rc;
    const bf16_t *x = (const bf16_t *)x_;
    bf16_t *y = (bf16_t *)y_;
    KD_REQUIRE(x && y && gamma && beta && save_mean && save_invstd, KD_ERR_INVALID, "kd_bn_nhwc_lp_fwd: null argument");
    KD_REQUIRE(ldx >= C && ldy >= C, KD_ERR_INVALID, "kd_bn_nhwc_lp_fwd: pixel stride below C");
    KD_REQUIRE(training || (running_mean && running_var), KD_ERR_INVALID, "kd_bn_nhwc_lp_fwd: eval mode needs the running statistics");
    KD_REQUIRE(!training || (workspace && workspace_bytes >= bn_lp_workspace(M, C)), KD_ERR_WORKSPACE, "kd_bn_nhwc_lp_fwd: workspace too small");
    const BnLpSel sel = bn_lp_select_fwd(x, ldx, y, ldy, M, C);
    KD_NOTE_PLUMBING(bn_lp_kernel_name(sel.kernel));
    hipStream_t s = (hipStream_t)stream;
    if (training) {
        if (sel.vec) launch_lp_fwd_stats<8>(sel, g, x, ldx, (float *)workspace, save_mean, save_invstd, running_mean, running_var, momentum, eps, s);
        else launch_lp_fwd_stats<1>(sel, g, x, ldx, (float *)workspace, save_mean, save_invstd, running_mean, running_var, momentum, eps, s);
        KD_CHECK_LAUNCH("kd_bn_nhwc_lp_fwd(stats)");
    } else {
        hipLaunchKernelGGL(bn_nhwc_eval_stats_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, (int)C, (const float *)running_mean,
                           (const float *)running_var, eps, save_mean, save_invstd);
        KD_CHECK_LAUNCH("kd_bn_nhwc_lp_fwd(eval)");
    }
    if (sel.vec)
        hipLaunchKernelGGL(bn_lp_apply_kernel<8>, dim3(sel.grid), dim3(TPB), 0, s, g, x, ldx, y, ldy, gamma, beta, (const float *)save_mean,
                           (const float *)save_invstd, (int)relu);
    else
        hipLaunchKernelGGL(bn_lp_apply_kernel<1>, dim3(sel.grid), dim3(TPB), 0, s, g, x, ldx, y, ldy, gamma, beta, (const float *)save_mean,
                           (const float *)save_invstd, (int)relu);
    KD_CHECK_LAUNCH("kd_bn_nhwc_lp_fwd(apply)");
    return KD_OK;
}

extern "C" int kd_bn_nhwc_lp_bwd(const void *gy_, int32_t ldg, const void *x_, int32_t ldx, const void *y_, int32_t ldy, const void *res_,
                                 int32_t ldres, void *dx_, int32_t lddx, int64_t M, int32_t C, const float *gamma, const float *save_mean,
                                 const float *save_invstd, float *dgamma, float *dbeta, int32_t accumulate, int32_t training, int32_t relu,
                                 void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    BnGeom g;
    if (int rc = geom(M, C, g, "kd_bn_nhwc_lp_bwd")) return rc;
    const bf16_t *gy = (const bf16_t *)gy_, *x = (const bf16_t *)x_, *y = relu ? (const bf16_t *)y_ : nullptr, *res = (const bf16_t *)res_;
    bf16_t *dx = (bf16_t *)dx_;
    KD_REQUIRE(gy && x && gamma && save_mean && save_invstd, KD_ERR_INVALID, "kd_bn_nhwc_lp_bwd: null argument");
    KD_REQUIRE(!relu || y, KD_ERR_INVALID, "kd_bn_nhwc_lp_bwd: the fused-ReLU backward needs the forward output");
    KD_REQUIRE(dx || dgamma || dbeta, KD_ERR_INVALID, "kd_bn_nhwc_lp_bwd: nothing requested");
    KD_REQUIRE(ldg >= C && ldx >= C && (!y || ldy >= C) && (!res || ldres >= C) && (!dx || lddx >= C), KD_ERR_INVALID,
               "kd_bn_nhwc_lp_bwd: pixel stride below C");
    const bool need_sums = (dx && training) || dgamma || dbeta;
    KD_REQUIRE(!need_sums || (workspace && workspace_bytes >= bn_lp_workspace(M, C)), KD_ERR_WORKSPACE, "kd_bn_nhwc_lp_bwd: workspace too small");
    const BnLpSel sel = bn_lp_select_bwd(gy, ldg, x, ldx, y, ldy, dx ? res : nullptr, ldres, dx, lddx, M, C);
    KD_NOTE_PLUMBING(bn_lp_kernel_name(sel.kernel));
    hipStream_t s = (hipStream_t)stream;
    float *sums = nullptr;
    if (need_sums) {
        float *part = (float *)workspace;
        sums = part + bn_lp_sums_offset(M, C);
        if (sel.vec)
            hipLaunchKernelGGL(bn_lp_grad_partial_kernel<8>, dim3(sel.part_x, sel.part_y), dim3(TPB), 0, s, g, gy, ldg, x, ldx, y, ldy, save_mean,
                               save_invstd, (int)relu, part);
        else
            hipLaunchKernelGGL(bn_lp_grad_partial_kernel<1>, dim3(sel.part_x, sel.part_y), dim3(TPB), 0, s, g, gy, ldg, x, ldx, y, ldy, save_mean,
                               save_invstd, (int)relu, part);
        KD_CHECK_LAUNCH("kd_bn_nhwc_lp_bwd(partial)");
        hipLaunchKernelGGL(bn_lp_grad_finish_kernel, dim3(sel.finish), dim3(TPB), 0, s, g, (const float *)part, sums, dgamma, dbeta, (int)accumulate);
        KD_CHECK_LAUNCH("kd_bn_nhwc_lp_bwd(finish)");
    }
    if (!dx) return KD_OK;
    if (sel.vec)
        hipLaunchKernelGGL(bn_lp_dx_kernel<8>, dim3(sel.grid), dim3(TPB), 0, s, g, gy, ldg, x, ldx, y, ldy, res, ldres, dx, lddx, gamma, save_mean,
                           save_invstd, (const float *)sums, (int)(training != 0), (int)relu);
    else
        hipLaunchKernelGGL(bn_lp_dx_kernel<1>, dim3(sel.grid), dim3(TPB), 0, s, g, gy, ldg, x, ldx, y, ldy, res, ldres, dx, lddx, gamma, save_mean,
                           save_invstd, (const float *)sums, (int)(training != 0), (int)relu);
    KD_CHECK_LAUNCH("kd_bn_nhwc_lp_bwd(dx)");
    return KD_OK;
}
