// The optimizer steps torch.optim.SGD, torch.optim.Adam and the reference's AdamW (utils/optim/radam.py:179-250) take, for many
// tensors in one launch (kd_optim_step_multi).  HBM-bound streaming kernels: every element of p, g and the state is read once
// and written once.  Batching follows radam_multi_kernel (losses.hip): the per-tensor pointers and constants travel by value in
// the kernel argument, a block finds its tensor by a short search in the block-prefix table, and a call with more tensors than
// one argument holds becomes several launches.  Nothing is allocated, copied or synchronised.
#include <math.h>

#include "kd_common.h"

namespace {

constexpr int OPT_BLK = 256 * 16;   // elements per block: four 16-byte accesses per lane and pointer

// kernel-side flags: the low bits are the public KD_OPT_* ones
enum { F_VEC = 1 << 8,    // every pointer of the tensor is 16-byte aligned: 16 bytes per lane, scalar tail
       F_MOM = 1 << 9,    // SGD: momentum != 0 (there is a momentum buffer)
       F_WD = 1 << 10 };  // weight_decay != 0

// What one rule needs per tensor: NPTR pointers (p, g, then the state) and NC fp32 constants.
template <int NPTR, int NC> struct OptBatch {
    static constexpr int MAXT = (4096 - 16) / (8 * NPTR + 8 + 4 + 4 + 4 * NC);
    float *ptr[NPTR][MAXT];   // [0] p, [1] g (only read), [2 ..] state
    long long n[MAXT];
    int blk0[MAXT + 1];       // first block of tensor t
    int flags[MAXT];
    float c[NC][MAXT];
    int count;
};

template <int RULE> struct Rule;
// c: lr, weight_decay, momentum, 1 - dampening
template <> struct Rule<KD_OPT_SGD> { static constexpr int NPTR = 3, NC = 4; };
// c: 1 - beta1, beta2, 1 - beta2, weight_decay, lr / bias_correction1, sqrt(bias_correction2), eps
template <> struct Rule<KD_OPT_ADAM> { static constexpr int NPTR = 5, NC = 7; };
// c: beta1, 1 - beta1, beta2, 1 - beta2, weight_decay * scheduled_lr, scheduled_lr * sqrt(bias_correction2) / bias_correction1, eps
template <> struct Rule<KD_OPT_ADAMW_REF> { static constexpr int NPTR = 4, NC = 7; };

template <int W> __device__ __forceinline__ void ldw(const float *q, float (&v)[W])
{
    if constexpr (W == 4) {
        const float4 a = *(const float4 *)q;
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
        v[0] = *q;
    }
}
template <int W> __device__ __forceinline__ void stw(float *q, const float (&v)[W])
{
    if constexpr (W == 4) *(float4 *)q = make_float4(v[0], v[1], v[2], v[3]);
    else *q = v[0];
}

// One element.  Every product and sum is written out (explicit fmaf, contraction off), so an element's result is the same
// whether the 16-byte or the scalar path stored it, and whatever its neighbours in the launch are.
template <int RULE, int NC>
__device__ __forceinline__ void optim_element(float &p, float g, float &s0, float &s1, float &s2, const float (&c)[NC], int flags)
{
#pragma clang fp contract(off)
    if constexpr (RULE == KD_OPT_SGD) {
        if (flags & KD_OPT_MAXIMIZE) g = -g;
        if (flags & F_WD) g = fmaf(c[1], p, g);
        if (flags & F_MOM) {
            s0 = (flags & KD_OPT_FIRST) ? g : fmaf(c[2], s0, c[3] * g);
            g = (flags & KD_OPT_NESTEROV) ? fmaf(c[2], s0, g) : s0;
        }
        p = fmaf(-c[0], g, p);
    } else if constexpr (RULE == KD_OPT_ADAM) {
        if (flags & KD_OPT_MAXIMIZE) g = -g;
        if (flags & F_WD) g = fmaf(c[3], p, g);
        s0 = fmaf(c[0], g - s0, s0);
        s1 = fmaf(c[1], s1, c[2] * g * g);
        float v = s1;
        if (flags & KD_OPT_AMSGRAD) {
            s2 = (s1 > s2 || s1 != s1) ? s1 : s2;   // torch.maximum: a NaN stays
            v = s2;
        }
        p = fmaf(-c[4], s0 / (sqrtf(v) / c[5] + c[6]), p);
    } else {
        s1 = fmaf(c[2], s1, c[3] * g * g);
        s0 = fmaf(c[0], s0, c[1] * g);
        if (flags & F_WD) p = fmaf(-c[4], p, p);
        p = fmaf(-c[5], s0 / (sqrtf(s1) + c[6]), p);
    }
}

// W consecutive elements at i: which state slots are read and written is the same for the whole tensor (rd / wr, bit per slot)
template <int RULE, int W, int NPTR, int NC>
__device__ __forceinline__ void optim_span(float *(&ptr)[NPTR], long long i, const float (&c)[NC], int flags, int rd, int wr)
{
    float P[W], G[W], S[3][W];
    ldw<W>(ptr[0] + i, P);
    ldw<W>(ptr[1] + i, G);
#pragma unroll
    for (int s = 0; s < NPTR - 2; ++s)
        if (rd >> s & 1) ldw<W>(ptr[2 + s] + i, S[s]);
#pragma unroll
    for (int q = 0; q < W; ++q) optim_element<RULE, NC>(P[q], G[q], S[0][q], S[1][q], S[2][q], c, flags);
    stw<W>(ptr[0] + i, P);
#pragma unroll
    for (int s = 0; s < NPTR - 2; ++s)
        if (wr >> s & 1) stw<W>(ptr[2 + s] + i, S[s]);
}

template <int RULE>
__global__ __launch_bounds__(256) void optim_multi_kernel(const OptBatch<Rule<RULE>::NPTR, Rule<RULE>::NC> b)
{
    constexpr int NPTR = Rule<RULE>::NPTR, NC = Rule<RULE>::NC;
    int lo = 0, hi = b.count - 1;
    while (lo < hi) {   // block-uniform
        const int mid = (lo + hi + 1) >> 1;
        if (b.blk0[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const int t = lo, flags = b.flags[t];
    float *ptr[NPTR];
    float c[NC];
#pragma unroll
    for (int s = 0; s < NPTR; ++s) ptr[s] = b.ptr[s][t];
#pragma unroll
    for (int q = 0; q < NC; ++q) c[q] = b.c[q][t];
    int rd, wr;
    if constexpr (RULE == KD_OPT_SGD) {
        wr = (flags & F_MOM) ? 1 : 0;
        rd = (flags & KD_OPT_FIRST) ? 0 : wr;     // the first step of a momentum buffer writes it and never reads it
    } else if constexpr (RULE == KD_OPT_ADAM) {
        rd = wr = (flags & KD_OPT_AMSGRAD) ? 7 : 3;
    } else {
        rd = wr = 3;
    }
    const long long base = (long long)((int)blockIdx.x - b.blk0[t]) * OPT_BLK;
    const long long end = min(b.n[t], base + OPT_BLK);
    long long vend = base;
    if (flags & F_VEC) {
        vend = base + ((end - base) & ~3LL);
        for (long long i = base + threadIdx.x * 4; i < vend; i += 256 * 4) optim_span<RULE, 4>(ptr, i, c, flags, rd, wr);
    }
    for (long long i = vend + threadIdx.x; i < end; i += 256) optim_span<RULE, 1>(ptr, i, c, flags, rd, wr);
}

// The constants of tensor t, computed in double as the Python of torch.optim / of the reference computes them, each rounded to
// float once.  Returns the kernel-side flags.
template <int RULE, int NC> int optim_constants(const kd_optim_tensor &t, float (&c)[NC])
{
    int flags = t.flags & (KD_OPT_FIRST | KD_OPT_NESTEROV | KD_OPT_AMSGRAD | KD_OPT_MAXIMIZE);
    if (t.weight_decay != 0.0) flags |= F_WD;
    if constexpr (RULE == KD_OPT_SGD) {
        if (t.momentum != 0.0) flags |= F_MOM;
        c[0] = (float)t.lr; c[1] = (float)t.weight_decay; c[2] = (float)t.momentum; c[3] = (float)(1.0 - t.dampening);
    } else {
        const double step = (double)t.step;
        const double bc1 = 1.0 - pow(t.beta1, step), bc2 = 1.0 - pow(t.beta2, step);
        if constexpr (RULE == KD_OPT_ADAM) {
            c[0] = (float)(1.0 - t.beta1); c[1] = (float)t.beta2; c[2] = (float)(1.0 - t.beta2); c[3] = (float)t.weight_decay;
            c[4] = (float)(t.lr / bc1); c[5] = (float)sqrt(bc2); c[6] = (float)t.eps;
        } else {
            const double slr = t.warmup > step ? 1e-8 + step * t.lr / t.warmup : t.lr;
            c[0] = (float)t.beta1; c[1] = (float)(1.0 - t.beta1); c[2] = (float)t.beta2; c[3] = (float)(1.0 - t.beta2);
            c[4] = (float)(t.weight_decay * slr); c[5] = (float)(slr * sqrt(bc2) / bc1); c[6] = (float)t.eps;
        }
    }
    return flags;
}

// the state slots rule RULE touches for tensor t (they must be there)
template <int RULE> int optim_slots(const kd_optim_tensor &t)
{
    if constexpr (RULE == KD_OPT_SGD) return t.momentum != 0.0 ? 1 : 0;
    else if constexpr (RULE == KD_OPT_ADAM) return (t.flags & KD_OPT_AMSGRAD) ? 3 : 2;
    else return 2;
}

template <int RULE> int optim_launch(const kd_optim_tensor *ts, int count, hipStream_t stream)
{
    typedef OptBatch<Rule<RULE>::NPTR, Rule<RULE>::NC> Batch;
    static_assert(sizeof(Batch) <= 4096, "kernel argument space");
    constexpr int NPTR = Rule<RULE>::NPTR;
    for (int i = 0; i < count; ++i) {
        const kd_optim_tensor &t = ts[i];
        KD_REQUIRE(t.p && t.g && t.n > 0, KD_ERR_INVALID, "kd_optim_step_multi: bad tensor %d", i);
        KD_REQUIRE(RULE == KD_OPT_SGD || t.step >= 1, KD_ERR_INVALID, "kd_optim_step_multi: tensor %d: step counts from 1", i);
        for (int s = 0; s < optim_slots<RULE>(t); ++s)
            KD_REQUIRE(t.state[s], KD_ERR_INVALID, "kd_optim_step_multi: tensor %d lacks state %d", i, s);
    }
    for (int done = 0; done < count;) {
        Batch b;
        int nb = 0, k = 0;
        for (; k < Batch::MAXT && done + k < count; ++k) {
            const kd_optim_tensor &t = ts[done + k];
            const long long blocks = (t.n + OPT_BLK - 1) / OPT_BLK;
            if (k > 0 && nb + blocks > 0x3fffffffLL) break;
            KD_REQUIRE(blocks <= 0x3fffffffLL, KD_ERR_UNSUPPORTED, "kd_optim_step_multi: tensor too large");
            float c[Rule<RULE>::NC];
            int flags = optim_constants<RULE>(t, c);
            const int slots = optim_slots<RULE>(t);
            bool vec = kd_aligned16(t.p) && kd_aligned16(t.g);
            b.ptr[0][k] = t.p;
            b.ptr[1][k] = const_cast<float *>(t.g);
            for (int s = 0; s < NPTR - 2; ++s) {
                b.ptr[2 + s][k] = s < slots ? t.state[s] : nullptr;
                if (s < slots) vec = vec && kd_aligned16(t.state[s]);
            }
            if (vec) flags |= F_VEC;
            b.n[k] = t.n;
            b.blk0[k] = nb;
            b.flags[k] = flags;
            for (int q = 0; q < Rule<RULE>::NC; ++q) b.c[q][k] = c[q];
            nb += (int)blocks;
        }
        b.blk0[k] = nb;
        b.count = k;
        if constexpr (RULE == KD_OPT_SGD) KD_NOTE_PLUMBING("optim_multi_kernel<sgd>");
        else if constexpr (RULE == KD_OPT_ADAM) KD_NOTE_PLUMBING("optim_multi_kernel<adam>");
        else KD_NOTE_PLUMBING("optim_multi_kernel<adamw_ref>");
        hipLaunchKernelGGL(optim_multi_kernel<RULE>, dim3((unsigned)nb), dim3(256), 0, stream, b);
        KD_CHECK_LAUNCH("kd_optim_step_multi");
        done += k;
    }
    return KD_OK;
}

}  // namespace

extern "C" int kd_optim_step_multi(int32_t rule, const kd_optim_tensor *ts, int32_t count, kd_stream_t stream)
{
    KD_REQUIRE(ts && count > 0, KD_ERR_INVALID, "kd_optim_step_multi: bad argument");
    switch (rule) {
    case KD_OPT_SGD: return optim_launch<KD_OPT_SGD>(ts, count, (hipStream_t)stream);
    case KD_OPT_ADAM: return optim_launch<KD_OPT_ADAM>(ts, count, (hipStream_t)stream);
    case KD_OPT_ADAMW_REF: return optim_launch<KD_OPT_ADAMW_REF>(ts, count, (hipStream_t)stream);
    default: break;
    }
    kd_set_error("kd_optim_step_multi: unknown rule %d", rule);
    return KD_ERR_INVALID;
}

extern "C" int kd_optim_launch_shape(int32_t rule, int32_t *max_tensors, int32_t *block_elems)
{
    KD_REQUIRE(max_tensors && block_elems, KD_ERR_INVALID, "kd_optim_launch_shape: bad argument");
    *block_elems = OPT_BLK;
    switch (rule) {
    case KD_OPT_SGD: *max_tensors = OptBatch<Rule<KD_OPT_SGD>::NPTR, Rule<KD_OPT_SGD>::NC>::MAXT; return KD_OK;
    case KD_OPT_ADAM: *max_tensors = OptBatch<Rule<KD_OPT_ADAM>::NPTR, Rule<KD_OPT_ADAM>::NC>::MAXT; return KD_OK;
    case KD_OPT_ADAMW_REF: *max_tensors = OptBatch<Rule<KD_OPT_ADAMW_REF>::NPTR, Rule<KD_OPT_ADAMW_REF>::NC>::MAXT; return KD_OK;
    default: break;
    }
    kd_set_error("kd_optim_launch_shape: unknown rule %d", rule);
    return KD_ERR_INVALID;
}
