// BatchNorm -> ReLU -> MaxPool2d(2, 2) of the CIFAR VGGs (models/cifar_models/vgg.py) as one pass over x that never stores the
// full-resolution activation (kd_bn_relu_maxpool2x2_fwd), and its backward, which recomputes the four activations of every window
// from x and routes the pooled gradient to the first maximum (kd_bn_relu_maxpool2x2_bwd).  fp32 NHWC views with a pixel stride.
//
// A thread owns whole 2x2 windows of V channels: V = 4 (one 16-B access per pixel) or V = 1.  The activation is
// a = max(fmaf(x - mean, gamma * invstd, beta), 0), the expression of bn_nhwc_core.h's apply kernel; without BatchNorm operands
// (gamma == NULL) the same code runs with mean = 0, scale = 1, shift = 0, which is exact.  The routed gradient g' of a window is
// gpooled at the FIRST position in (ky, kx) order that holds the window's maximum, where that maximum is positive, and 0 at the
// other positions: what MaxPool2d's backward followed by ReLU's gives.  An odd last row or column belongs to no window.
//   forward   grid-stride over windows x C / V: four loads, one store; the items of window 0 update the running statistics.
//   backward  stage 1 (one workgroup per POOL_WINS windows x 64 channels): part[block][0][c] = sum g', part[block][1][c] = sum g' xhat,
//             a thread's windows in ascending order, then bn_nhwc_core.h's fold over the window lanes;
//             stage 2: bn_nhwc_core.h's bn_nhwc_grad_finish_kernel, fp64 chains in a fixed order -> sums, dbeta, dgamma;
//             dx: grid-stride over cells (the windows plus the partial ones of an odd row / column) x C / V, every pixel of x once:
//             dx = gamma invstd (g' - [training] (sum g' + xhat sum g' xhat) / M), M = N H W.
// No atomics; the partials live in the caller's workspace (kd_bn_nhwc_workspace(M, C) bytes hold them, pool_select.h).  Which
// instantiation runs, on what grids, is pool_select.h's decision.
#include "pool_select.h"
#include "bn_nhwc_core.h"

namespace {

static_assert(POOL_TPB == TPB && POOL_CBLOCK == 64 && POOL_FINISH_CH == BN_BWD_FINISH_CH && POOL_VEC * sizeof(float) == POOL_VEC_BYTES,
              "pool_select.h plans the grids for bn_nhwc_core.h's blocking");
static_assert(POOL_WINS * 4 >= BN_ROWS, "no more window blocks than row blocks: the partials of a pass fit the BatchNorm workspace");

struct PoolGeom {
    int N, H, W, C;
    int Ho, Wo;             // pooled map
    int He, We;             // cells per column / row: ceil(H / 2), ceil(W / 2)
    long long windows;      // N Ho Wo
    long long cells;        // N He We
};

// The BN operands of a thread's V channels; without BatchNorm the identity.
template <int V> struct PoolChan {
    float mu[V], k[V], b[V], is[V];
    __device__ __forceinline__ PoolChan(int c0, const float *gamma, const float *beta, const float *mean, const float *invstd)
    {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            mu[j] = gamma ? mean[c0 + j] : 0.f;
            is[j] = gamma ? invstd[c0 + j] : 1.f;
            k[j] = gamma ? gamma[c0 + j] * is[j] : 1.f;
            b[j] = gamma ? beta[c0 + j] : 0.f;
        }
    }
    __device__ __forceinline__ float act(int j, float x) const { return fmaxf(fmaf(x - mu[j], k[j], b[j]), 0.f); }
};

// index (0 .. 3, ky * 2 + kx) of the first maximum of a window's activations, or -1 where none is positive
__device__ __forceinline__ int first_max(float a0, float a1, float a2, float a3)
{
    int at = 0;
    float best = a0;
    if (a1 > best) { best = a1; at = 1; }
    if (a2 > best) { best = a2; at = 2; }
    if (a3 > best) { best = a3; at = 3; }
    return best > 0.f ? at : -1;
}

template <int V>
__global__ __launch_bounds__(TPB) void pool_fwd_kernel(PoolGeom g, const float *__restrict__ x, int ldx, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, const float *__restrict__ mean,
                                                       const float *__restrict__ invstd, float *__restrict__ y, int ldy,
                                                       const float *__restrict__ var_unb, float *__restrict__ run_mean,
                                                       float *__restrict__ run_var, float momentum)
{
    const int cv = g.C / V;
    const long long total = g.windows * cv;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const long long w = i / cv;
        const int c0 = (int)(i - w * cv) * V;
        const int wo = (int)(w % g.Wo), ho = (int)((w / g.Wo) % g.Ho);
        const long long n = w / ((long long)g.Wo * g.Ho);
        const PoolChan<V> ch(c0, gamma, beta, mean, invstd);
        if (w == 0 && gamma) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if (run_mean) run_mean[c0 + j] = bn_running_update(run_mean[c0 + j], momentum, ch.mu[j]);
                if (run_var) run_var[c0 + j] = bn_running_update(run_var[c0 + j], momentum, var_unb[c0 + j]);
            }
        }
        const float *p = x + ((n * g.H + 2 * ho) * g.W + 2 * wo) * ldx + c0;
        float v[4][V], o[V];
        ldv<V>(p, v[0]);
        ldv<V>(p + ldx, v[1]);
        ldv<V>(p + (long long)g.W * ldx, v[2]);
        ldv<V>(p + (long long)(g.W + 1) * ldx, v[3]);
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = fmaxf(fmaxf(ch.act(j, v[0][j]), ch.act(j, v[1][j])), fmaxf(ch.act(j, v[2][j]), ch.act(j, v[3][j])));
        stv<V>(y + w * ldy + c0, o);
    }
}

// stage 1 backward: part[wb][0][c] = sum g', part[wb][1][c] = sum g' xhat over the block's windows
template <int V>
__global__ __launch_bounds__(TPB) void pool_grad_partial_kernel(PoolGeom g, const float *__restrict__ x, int ldx, const float *__restrict__ gp,
                                                                int ldg, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                const float *__restrict__ mean, const float *__restrict__ invstd,
                                                                float *__restrict__ part)
{
    constexpr int CL = 64 / V, WL = TPB / CL;
    __shared__ float sh[2][4][64];
    const int tx = threadIdx.x % CL, ty = threadIdx.x / CL;
    const int c0 = blockIdx.y * 64 + tx * V, wb = blockIdx.x;
    const long long w0 = (long long)wb * POOL_WINS;
    const long long w1 = w0 + POOL_WINS < g.windows ? w0 + POOL_WINS : g.windows;
    float s[2][V] = {};
    if (c0 < g.C) {
        const PoolChan<V> ch(c0, gamma, beta, mean, invstd);
        for (long long w = w0 + ty; w < w1; w += WL) {
            const int wo = (int)(w % g.Wo), ho = (int)((w / g.Wo) % g.Ho);
            const long long n = w / ((long long)g.Wo * g.Ho);
            const float *p = x + ((n * g.H + 2 * ho) * g.W + 2 * wo) * ldx + c0;
            float v[4][V], gv[V];
            ldv<V>(p, v[0]);
            ldv<V>(p + ldx, v[1]);
            ldv<V>(p + (long long)g.W * ldx, v[2]);
            ldv<V>(p + (long long)(g.W + 1) * ldx, v[3]);
            ldv<V>(gp + w * ldg + c0, gv);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int at = first_max(ch.act(j, v[0][j]), ch.act(j, v[1][j]), ch.act(j, v[2][j]), ch.act(j, v[3][j]));
                const float xm = at == 1 ? v[1][j] : at == 2 ? v[2][j] : at == 3 ? v[3][j] : v[0][j];
                const float t = at < 0 ? 0.f : gv[j];
                s[0][j] += t;
                s[1][j] = fmaf(t, (xm - ch.mu[j]) * ch.is[j], s[1][j]);
            }
        }
    }
    float tot[2];
    fold_row_lanes<V, 2>(s, sh, tot);
    const int c = blockIdx.y * 64 + threadIdx.x;
    if (threadIdx.x < 64 && c < g.C) {
        float *p = part + (size_t)wb * 2 * g.C;
        p[c] = tot[0];
        p[g.C + c] = tot[1];
    }
}

// dx of every pixel once: a cell is a window, or the part of one an odd last row / column leaves (no gradient is routed there)
template <int V>
__global__ __launch_bounds__(TPB) void pool_bwd_kernel(PoolGeom g, const float *__restrict__ x, int ldx, const float *__restrict__ gp, int ldg,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                                       const float *__restrict__ mean, const float *__restrict__ invstd,
                                                       const float *__restrict__ sums, float *__restrict__ dx, int lddx, int training)
{
    const int cv = g.C / V;
    const long long total = g.cells * cv;
    const float inv_m = (float)(1.0 / ((double)g.N * g.H * g.W));
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const long long cell = i / cv;
        const int c0 = (int)(i - cell * cv) * V;
        const int we = (int)(cell % g.We), he = (int)((cell / g.We) % g.He);
        const long long n = cell / ((long long)g.We * g.He);
        const PoolChan<V> ch(c0, gamma, beta, mean, invstd);
        const bool right = 2 * we + 1 < g.W, below = 2 * he + 1 < g.H, whole = right && below;
        const bool live[4] = {true, right, below, whole};
        const long long pix = (n * g.H + 2 * he) * g.W + 2 * we;
        const long long off[4] = {0, 1, g.W, (long long)g.W + 1};
        float v[4][V] = {}, gv[V] = {};
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (live[q]) ldv<V>(x + (pix + off[q]) * ldx + c0, v[q]);
        if (whole) ldv<V>(gp + ((n * g.Ho + he) * g.Wo + we) * ldg + c0, gv);
        int at[V];
        float mb[V], mg[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            at[j] = whole ? first_max(ch.act(j, v[0][j]), ch.act(j, v[1][j]), ch.act(j, v[2][j]), ch.act(j, v[3][j])) : -1;
            mb[j] = training ? sums[c0 + j] * inv_m : 0.f;
            mg[j] = training ? sums[g.C + c0 + j] * inv_m : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!live[q]) continue;
            float o[V];
#pragma unroll
            for (int j = 0; j < V; ++j) {
                float t = at[j] == q ? gv[j] : 0.f;
                if (training) t = t - mb[j] - (v[q][j] - ch.mu[j]) * ch.is[j] * mg[j];
                o[j] = ch.k[j] * t;
            }
            stv<V>(dx + (pix + off[q]) * lddx + c0, o);
        }
    }
}

bool aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }

int pool_geom(int32_t N, int32_t H, int32_t W, int32_t C, int32_t ldx, int32_t ldo, PoolGeom &g, const char *who)
{
    KD_REQUIRE(pool_shape_ok(N, H, W, C, ldx, ldo), KD_ERR_INVALID, "%s: N = %d, H = %d, W = %d, C = %d, pixel strides %d / %d", who, (int)N, (int)H,
               (int)W, (int)C, (int)ldx, (int)ldo);
    const long long M = (long long)N * H * W;
    KD_REQUIRE(M < (1ll << 31) && (M + ROWS - 1) / ROWS < 65536 && (C + 63) / 64 < 65536, KD_ERR_UNSUPPORTED,
               "%s: M = %lld, C = %d exceed the supported size", who, M, (int)C);
    g.N = N; g.H = H; g.W = W; g.C = C;
    g.Ho = H / 2; g.Wo = W / 2; g.He = (H + 1) / 2; g.We = (W + 1) / 2;
    g.windows = pool_windows(N, H, W);
    g.cells = pool_cells(N, H, W);
    return KD_OK;
}

}  // namespace

extern "C" int kd_bn_relu_maxpool2x2_fwd(const float *x, int32_t ldx, int32_t N, int32_t H, int32_t W, int32_t C, const float *gamma,
                                         const float *beta, const float *mean, const float *invstd, float *y, int32_t ldy,
                                         const float *var_unbiased, float *running_mean, float *running_var, float momentum, kd_stream_t stream)
{
    const char *who = "kd_bn_relu_maxpool2x2_fwd";
    KD_REQUIRE(x && y, KD_ERR_INVALID, "%s: null argument", who);
    KD_REQUIRE(!gamma ? (!beta && !mean && !invstd && !running_mean && !running_var) : (beta && mean && invstd), KD_ERR_INVALID,
               "%s: gamma, beta, mean and invstd come together (all NULL: no BatchNorm)", who);
    KD_REQUIRE(!running_var || var_unbiased, KD_ERR_INVALID, "%s: running_var without var_unbiased", who);
    PoolGeom g;
    if (int rc = pool_geom(N, H, W, C, ldx, ldy, g, who)) return rc;
    KD_REQUIRE(ldy >= C, KD_ERR_INVALID, "%s: y pixel stride %d below C = %d", who, (int)ldy, (int)C);
    KD_REQUIRE(aligned4(x) && aligned4(y) && aligned4(gamma) && aligned4(beta) && aligned4(mean) && aligned4(invstd) && aligned4(var_unbiased) &&
                   aligned4(running_mean) && aligned4(running_var),
               KD_ERR_INVALID, "%s: an operand is not aligned to its element", who);
    const PoolSel sel = pool_select_fwd(N, H, W, C, x, ldx, y, ldy);
    KD_NOTE_PLUMBING(pool_kernel_name(sel.kernel));
    hipStream_t s = (hipStream_t)stream;
    const auto fwd = sel.vec == 1 ? pool_fwd_kernel<1> : pool_fwd_kernel<POOL_VEC>;
    hipLaunchKernelGGL(fwd, dim3(sel.grid), dim3(TPB), 0, s, g, x, ldx, gamma, beta, mean, invstd, y, ldy, var_unbiased, running_mean, running_var,
                       momentum);
    KD_CHECK_LAUNCH(who);
    return KD_OK;
}

extern "C" int kd_bn_relu_maxpool2x2_bwd(const float *x, int32_t ldx, const float *gpooled, int32_t ldg, int32_t N, int32_t H, int32_t W, int32_t C,
                                         const float *gamma, const float *beta, const float *mean, const float *invstd, float *dx, int32_t lddx,
                                         float *dgamma, float *dbeta, int32_t training, void *workspace, size_t workspace_bytes,
                                         kd_stream_t stream)
{
    const char *who = "kd_bn_relu_maxpool2x2_bwd";
    KD_REQUIRE(x && gpooled, KD_ERR_INVALID, "%s: null argument", who);
    KD_REQUIRE(!gamma ? (!beta && !mean && !invstd && !dgamma && !dbeta && dx) : (beta && mean && invstd && dgamma && dbeta), KD_ERR_INVALID,
               "%s: gamma, beta, mean, invstd, dgamma and dbeta come together (all NULL: no BatchNorm, dx alone)", who);
    PoolGeom g;
    if (int rc = pool_geom(N, H, W, C, ldx, ldg, g, who)) return rc;
    KD_REQUIRE(ldg >= C && (!dx || lddx >= C), KD_ERR_INVALID, "%s: pixel strides %d / %d below C = %d", who, (int)ldg, (int)lddx, (int)C);
    KD_REQUIRE(aligned4(x) && aligned4(gpooled) && aligned4(gamma) && aligned4(beta) && aligned4(mean) && aligned4(invstd) && aligned4(dx) &&
                   aligned4(dgamma) && aligned4(dbeta),
               KD_ERR_INVALID, "%s: an operand is not aligned to its element", who);
    const PoolSel sel = pool_select_bwd(gamma != nullptr, N, H, W, C, x, ldx, gpooled, ldg, dx, lddx);
    KD_REQUIRE(sel.workspace_bytes == 0 || (workspace && workspace_bytes >= sel.workspace_bytes), KD_ERR_WORKSPACE, "%s: workspace too small", who);
    KD_NOTE_PLUMBING(pool_kernel_name(sel.kernel));
    hipStream_t s = (hipStream_t)stream;
    const int tr = gamma && training != 0;
    float *sums = nullptr;
    if (gamma) {
        float *part = (float *)workspace;
        sums = part + sel.sums_offset;
        const auto partial = sel.vec == 1 ? pool_grad_partial_kernel<1> : pool_grad_partial_kernel<POOL_VEC>;
        hipLaunchKernelGGL(partial, dim3(sel.part_x, sel.part_y), dim3(TPB), 0, s, g, x, ldx, gpooled, ldg, gamma, beta, mean, invstd, part);
        KD_CHECK_LAUNCHF("%s(partial)", who);
        BnGeom bg;
        bg.M = g.windows; bg.C = C; bg.nrb = sel.nwb;
        hipLaunchKernelGGL(bn_nhwc_grad_finish_kernel, dim3(sel.finish), dim3(TPB), 0, s, bg, (const float *)part, sums, dgamma, dbeta, 0);
        KD_CHECK_LAUNCHF("%s(finish)", who);
    }
    if (!dx) return KD_OK;
    const auto dxk = sel.vec == 1 ? pool_bwd_kernel<1> : pool_bwd_kernel<POOL_VEC>;
    hipLaunchKernelGGL(dxk, dim3(sel.grid), dim3(TPB), 0, s, g, x, ldx, gpooled, ldg, gamma, beta, mean, invstd, (const float *)sums, dx, lddx, tr);
    KD_CHECK_LAUNCH(who);
    return KD_OK;
}
