// BatchNorm2d on NHWC views for the Wide-ResNet-28-10 CIFAR path (models/cifar_models/wrn.py): 16 / 160 / 320 / 640 channels at
// 32x32 .. 8x8, the student in TRAINING mode (classification_trainer.py:21) so every BN of it -- frozen ones
// included -- normalises with batch statistics between two MFMA convolutions.  fp32 storage (kd_bn_nhwc_*) and bf16 storage
// (kd_bn_nhwc_lp_*) are one implementation, bn_nhwc_core.h's, instantiated for float and bf16_t; the kernel and grids of a call
// are bn_select.h's decision.  The entry points below only cast and call.
#include "bn_nhwc_core.h"

extern "C" size_t kd_bn_nhwc_workspace(int64_t M, int32_t C)
{
    return bn_workspace(M, C);
}

extern "C" size_t kd_bn_nhwc_lp_workspace(int64_t M, int32_t C)
{
    return bn_workspace(M, C);
}

extern "C" int kd_bn_nhwc_fwd(const float *x, int32_t ldx, float *y, int32_t ldy, int64_t M, int32_t C, const float *gamma,
                              const float *beta, float *save_mean, float *save_invstd, float *running_mean, float *running_var,
                              float momentum, float eps, int32_t training, int32_t relu, void *workspace, size_t workspace_bytes,
                              kd_stream_t stream)
{
    return bn_forward<float>("kd_bn_nhwc_fwd", x, ldx, y, ldy, M, C, gamma, beta, save_mean, save_invstd, running_mean, running_var, momentum, eps,
                             training, relu, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int kd_bn_nhwc_lp_fwd(const void *x, int32_t ldx, void *y, int32_t ldy, int64_t M, int32_t C, const float *gamma, const float *beta,
                                 float *save_mean, float *save_invstd, float *running_mean, float *running_var, float momentum, float eps,
                                 int32_t training, int32_t relu, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    return bn_forward<bf16_t>("kd_bn_nhwc_lp_fwd", (const bf16_t *)x, ldx, (bf16_t *)y, ldy, M, C, gamma, beta, save_mean, save_invstd, running_mean,
                              running_var, momentum, eps, training, relu, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int kd_bn_nhwc_bwd(const float *gy, int32_t ldg, const float *x, int32_t ldx, const float *y, int32_t ldy,
                              const float *res, int32_t ldres, float *dx, int32_t lddx, int64_t M, int32_t C, const float *gamma,
                              const float *save_mean, const float *save_invstd, float *dgamma, float *dbeta, int32_t accumulate,
                              int32_t training, int32_t relu, void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    return bn_backward<float>("kd_bn_nhwc_bwd", gy, ldg, x, ldx, y, ldy, res, ldres, dx, lddx, M, C, gamma, save_mean, save_invstd, dgamma, dbeta,
                              accumulate, training, relu, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int kd_bn_nhwc_lp_bwd(const void *gy, int32_t ldg, const void *x, int32_t ldx, const void *y, int32_t ldy, const void *res,
                                 int32_t ldres, void *dx, int32_t lddx, int64_t M, int32_t C, const float *gamma, const float *save_mean,
                                 const float *save_invstd, float *dgamma, float *dbeta, int32_t accumulate, int32_t training, int32_t relu,
                                 void *workspace, size_t workspace_bytes, kd_stream_t stream)
{
    return bn_backward<bf16_t>("kd_bn_nhwc_lp_bwd", (const bf16_t *)gy, ldg, (const bf16_t *)x, ldx, (const bf16_t *)y, ldy, (const bf16_t *)res,
                               ldres, (bf16_t *)dx, lddx, M, C, gamma, save_mean, save_invstd, dgamma, dbeta, accumulate, training, relu,
                               workspace, workspace_bytes, (hipStream_t)stream);
}
