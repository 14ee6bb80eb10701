// The bilinear resampling rule of the library, stated once: the geometry the host hands a kernel, the source coordinate of an
// output index, the blend, and -- for the adjoint kernels, which gather -- the candidate outputs of a source index and the weight
// each contributes.  Every kernel that resamples (trunk_ops.hip, bwd_ops.hip, hrnet_ops.hip, losses.hip, gscnn_ops.hip) and every
// selector that fills a geometry (plumb_select.h, loss_select.h, gscnn_select.h) calls these.  Plain C++ for the host and the
// device alike: tests/test_resample_host.py holds the host build against its own float32 restatement, bit for bit.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define RESAMPLE_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define RESAMPLE_FN static inline
#endif

// (h, w) -> (H, W).  src = o * s + off along each axis: align_corners: s = (i-1)/(O-1) (0 when O == 1), off = 0; otherwise
// s = i/O, off = 0.5 s - 0.5, i.e. src = (o + 0.5) * i/O - 0.5.
struct ResampleGeom { float sh, sw, oh, ow; };
RESAMPLE_FN ResampleGeom resample_geom(int h, int w, int H, int W, int align_corners)
{
    ResampleGeom g;
    g.sh = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f;
    g.sw = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    g.oh = 0.f; g.ow = 0.f;
    if (!align_corners) {
        g.sh = (float)h / (float)H; g.sw = (float)w / (float)W;
        g.oh = 0.5f * g.sh - 0.5f; g.ow = 0.5f * g.sw - 0.5f;
    }
    return g;
}

// output index o of an axis with I source samples: src = max(o * s + off, 0), i0 = min(floor(src), I - 1),
// i1 = min(i0 + 1, I - 1), f = src - i0.  (o * s + off is plain C: the device compiler contracts it to one fused multiply-add,
// a host build without contraction rounds the product first.  An explicit fmaf moved instructions in kernels that call this.)
RESAMPLE_FN void resample_split(float src, int I, int &i0, int &i1, float &f)
{
    i0 = (int)src; i0 = i0 > I - 1 ? I - 1 : i0;
    i1 = i0 + 1 < I ? i0 + 1 : I - 1;
    f = src - (float)i0;
}
RESAMPLE_FN void resample_src(int o, float s, float off, int I, int &i0, int &i1, float &f)
{
    resample_split(fmaxf(o * s + off, 0.f), I, i0, i1, f);
}
// align_corners callers whose off is 0 by construction: the same values, without an addition the compiler may not drop (-0)
RESAMPLE_FN void resample_src(int o, float s, int I, int &i0, int &i1, float &f)
{
    resample_split(fmaxf(o * s, 0.f), I, i0, i1, f);
}

// y[o] = (1 - f) x[i0] + f x[i1]
RESAMPLE_FN float resample_lerp(float f, float a, float b) { return (1.f - f) * a + f * b; }

// The outputs [lo, hi] that may read source index i, bracketed generously (s == 0: all of them): a gather over them that weighs
// each by resample_adjoint_weight is the adjoint of the forward, whatever the rounding of resample_src.
RESAMPLE_FN void resample_adjoint_range(int i, float s, float off, int O, int &lo, int &hi)
{
    if (s > 0.f) {
        const float inv = 1.f / s;
        lo = (int)(((float)(i - 1) - off) * inv) - 1;
        hi = (int)(((float)(i + 1) - off) * inv) + 2;
    } else {
        lo = 0; hi = O - 1;
    }
    lo = lo > 0 ? lo : 0;
    hi = hi < O - 1 ? hi : O - 1;
}

// what output o reads of source index i: (1 - f) if i0(o) == i, plus f if i1(o) == i
RESAMPLE_FN float resample_weight_of(int i, int i0, int i1, float f)
{
    float wgt = 0.f;
    if (i0 == i) wgt += 1.f - f;
    if (i1 == i) wgt += f;
    return wgt;
}
RESAMPLE_FN float resample_adjoint_weight(int o, int i, float s, float off, int I)
{
    int i0, i1; float f;
    resample_src(o, s, off, I, i0, i1, f);
    return resample_weight_of(i, i0, i1, f);
}
RESAMPLE_FN float resample_adjoint_weight(int o, int i, float s, int I)      // align_corners, as resample_src without an offset
{
    int i0, i1; float f;
    resample_src(o, s, I, i0, i1, f);
    return resample_weight_of(i, i0, i1, f);
}
