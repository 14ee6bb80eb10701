/*
 * kdcc.h -- C-ABI of libkdcc_hip.so: the MI355X (gfx950) kernels behind the
 * KD train step of lehduong/Knowledge-Distillation-by-Replacing-Cheap-Conv.
 *
 * The reference has no FFI / operator ABI: its hot path is Python classes
 * resolved by name (parse_config.py:80-93 `init_obj`; train.py:38-71) that
 * bottom out in torch.nn.functional calls.  Each entry point below replaces
 * the torch call(s) cited next to it; the Python host mirror
 * (knowledge-distillation-by-replacing-cheap-conv_amd/) keeps the reference's
 * class names and binds these symbols with ctypes.
 *
 * Conventions
 *  - plain pointers and sizes only; the caller owns every buffer (device memory);
 *    the library allocates nothing persistent and keeps no state;
 *  - all work is enqueued on the hipStream_t passed as `stream` (never the
 *    default stream implicitly, never a synchronisation);
 *  - return 0 on success, a negative KD_ERR_* otherwise; never throws;
 *    kd_last_error() returns a thread-local message for the last failure;
 *  - activations are NHWC ("channels last"): element (n,h,w,c) of a view with
 *    pixel stride `ld` lives at base[((n*H + h)*W + w)*ld + c]; ld >= C lets a
 *    kernel read / write a channel slice of a wider buffer (concat-free ASPP
 *    and decoder, deeplabv3.py:74,157);
 *  - dtype KD_BF16: bf16 storage, fp32 accumulate (the measured path);
 *    dtype KD_F32: fp32 storage, exact-fp32 MFMA (the parity path, 1e-3 gate).
 */
#ifndef KDCC_H
#define KDCC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *kd_stream_t; /* hipStream_t */

enum { KD_F32 = 0, KD_BF16 = 1 };
enum {
    KD_OK = 0,
    KD_ERR_INVALID = -1,     /* bad descriptor / null pointer / misalignment */
    KD_ERR_UNSUPPORTED = -2, /* shape outside what the kernels implement */
    KD_ERR_WORKSPACE = -3,   /* workspace too small */
    KD_ERR_HIP = -4          /* launch failed (hipGetLastError) */
};

int kd_version(void);
const char *kd_last_error(void);

/* ---------------------------------------------------------------- dense conv
 * Implicit-GEMM convolution on MFMA (im2col tile gathered straight into LDS).
 * Replaces nn.Conv2d forward at models/encoders/wider_resnet.py:124-167,
 * models/deeplabv3/deeplabv3.py:46-55,127-137 and the 1x1 `pointwise_conv` of
 * models/students/transform_blocks/depthwise_separable_conv.py:9, together
 * with the BN(eval)+ReLU (wider_resnet.py:43-48) and in-place residual add
 * (wider_resnet.py:181) that surround them, which are fused into the epilogue.
 * The same entry point computes the input gradient (autograd of those calls,
 * reached from loss.backward(), trainer/layerwise_trainer.py:235) when given
 * weights packed by kd_pack_conv_weight(..., KD_PACK_DGRAD) and the gradient as
 * `x`: for stride 1 the dgrad of a conv is a conv with flipped taps.
 *
 * Requirements: kh*kw in {1, 9}; Cin % 64 == 0 (bf16) or % 32 == 0 (f32);
 * x and w 16-byte aligned, ldx*sizeof(elem) % 16 == 0.
 * w: packed [Cout][kh][kw][Cin] in `dtype`.
 */
typedef struct kd_conv_desc {
    int32_t dtype;
    int32_t N, H, W, Cin; /* input view */
    int32_t Ho, Wo, Cout; /* output view */
    int32_t kh, kw, stride, pad, dil;
    int32_t ldx;          /* input pixel stride, elements */
} kd_conv_desc;

/* Epilogue, applied per output element (m = pixel, c = output channel):
 *   v = acc
 *   if res_pre   v += res_pre[m*ld_res_pre + c]
 *   if mask      v = mask[m*ld_mask + c] > 0 ? v * (mask_scale ? mask_scale[c] : 1) : 0
 *   if res_post  v += res_post[m*ld_res_post + c]
 *   if out_raw   out_raw[m*ld_raw + c] = v            (as float when raw_f32 != 0)
 *   if out_act   a = v * (act_scale ? act_scale[c] : 1) + (act_shift ? act_shift[c] : 0);
 *                out_act[m*ld_act + c] = act_relu ? max(a, 0) : a
 * forward:  res_pre = shortcut, out_raw = block output / hint, out_act = input of the next conv
 *           (next layer's eval-mode BN folded to scale/shift, + ReLU);
 * backward: mask = the saved activated tensor, mask_scale = that BN's scale
 *           (d relu(bn(x)) / dx), res_post = gradient arriving over the identity shortcut.
 */
typedef struct kd_conv_epilogue {
    const void *res_pre;  int32_t ld_res_pre;
    const void *mask;     int32_t ld_mask;     const float *mask_scale;
    const void *res_post; int32_t ld_res_post;
    void *out_raw;        int32_t ld_raw;      int32_t raw_f32;
    void *out_act;        int32_t ld_act;      const float *act_scale; const float *act_shift; int32_t act_relu;
    float *bn_sums;       /* optional, with `mask`: [M/128][2][Cout] fp32 partial sums over blocks of 128 output pixels of
                             g = (mask > 0 ? v * mask_scale : 0) and of g * mask -- the eval-mode BN parameter gradients'
                             reductions, taken where the input gradient is produced instead of by kd_channel_sums reading it
                             back.  Only the kernels kd_conv2d_bn_sums_rows() reports write it; finish with kd_bn_sums_finish.
                             WITHOUT `mask` (forward, round 6): part[r][0][c] = sum over the 128 pixels of row block r of the
                             values stored to out_raw, part[r][1][c] = 0 -- the global average pool of the ASPP image-pooling branch
                             (models/deeplabv3/deeplabv3.py:59-62) taken where its input is produced; kd_aspp_image_pool_sums
                             consumes the rows.  Only the ping-pong 1x1 kernel with no epilogue operand and out_raw alone. */
    /* Optional, round 6: a 1x1 classifier applied to the activation INSTEAD of storing it (out_raw and out_act NULL):
     *   cls_out[m][c] = sum_k bf16(act(scale[k] * v[m][k] + shift[k])) * cls_w[c][k],  c < ncls <= 32, fp32, pixel stride ld_cls floats;
     * cls_w is a [32][Cout] matrix in the conv's dtype, rows >= ncls zero (kd_pack_conv_weight of the 1x1 weight padded to 32 outputs).
     * The reference's `final` head (models/deeplabv3/deeplabv3.py:127-139: conv3x3 -> BN -> ReLU -> conv1x1 onto the classes) where nothing
     * else reads the 256-channel activation: it is neither written nor read back.  Same bf16 activation and bf16 weights as the
     * two-launch form, fp32 summation in another order.  Only conv_row_lw_kernel (bf16 3x3 / stride 1 / 'same', Cout == 256, no epilogue
     * operand, no bn_sums); kd_conv2d_cls_supported() says whether (d, ep) selects it, kd_conv2d_fwd refuses otherwise. */
    const void *cls_w;    float *cls_out;      int32_t ld_cls;      int32_t ncls;
} kd_conv_epilogue;
int32_t kd_conv2d_cls_supported(const kd_conv_desc *d, const kd_conv_epilogue *ep);

int kd_conv2d_fwd(const kd_conv_desc *d, const void *x, const void *w_packed,
                  const kd_conv_epilogue *ep, kd_stream_t stream);
/* Rows of `bn_sums` partials (one per 128 output pixels) the kernel kd_conv2d_fwd selects for (d, ep) writes, or 0 when that
 * kernel does not produce them -- the caller then leaves ep->bn_sums NULL (kd_conv2d_fwd refuses it otherwise) and takes the
 * sums with kd_channel_sums from the stored gradient.  The reference gets these reductions from autograd of
 * bn -> relu in IdentityResidualBlock (models/encoders/wider_resnet.py:124-167, reached from loss.backward(),
 * trainer/layerwise_trainer.py:235).
 * kd_bn_sums_finish: s1[c] = sum_r part[r][0][c], s2[c] = sum_r part[r][1][c] in a fixed order (fp64 accumulators; more than
 *   256 rows go through a first stage of 64- or 256-row chunks in `workspace`). */
int32_t kd_conv2d_bn_sums_rows(const kd_conv_desc *d, const kd_conv_epilogue *ep);
size_t kd_bn_sums_finish_workspace(int32_t rows, int32_t C);
int kd_bn_sums_finish(const float *part, int32_t rows, int32_t C, float *s1, float *s2, void *workspace, size_t workspace_bytes,
                      kd_stream_t stream);

/* K-concatenated 1x1 convolution: y = epilogue([x | x2] . w_cat^T) with ONE accumulator chain over K = d->Cin + Cin2 -- the two
 * 1x1 convs that land on the same tensor in the bottleneck blocks of WRN-38 (models/encoders/wider_resnet.py:143-182:
 * `out = self.convs(bn1); out.add_(shortcut)` with `shortcut = self.proj_conv(bn1)`: conv3 and proj_conv in mod6 / mod7), and in
 * their backward the input gradients of conv1 and proj_conv, which both land on bn1's output.  The shortcut tensor is never
 * written and read back and one wide epilogue disappears.  d describes the FIRST source (N,H,W,Cin,ldx; 1x1, stride 1, pad 0,
 * bf16); x2 is an (N,H,W,Cin2) view with pixel stride ldx2; w_cat is [Cout][Cin + Cin2] in `dtype` (the two packed weights
 * concatenated along K).  Runs on the persistent 256 x 256 ping-pong kernel only: kd_conv1x1_dual_supported() says whether (d,
 * Cin2, ep) selects it (M % 256 == 0, Cout % 256 == 0, >= 224 tiles, 16-B friendly epilogue); otherwise KD_ERR_UNSUPPORTED and
 * the caller runs the two convs (the second with res_pre).  Same values as those two launches up to the bf16 rounding of the
 * intermediate (the concatenated form rounds once). */
int32_t kd_conv1x1_dual_supported(const kd_conv_desc *d, int32_t Cin2, int32_t ldx2, const kd_conv_epilogue *ep);
int kd_conv1x1_dual_fwd(const kd_conv_desc *d, const void *x, const void *x2, int32_t Cin2, int32_t ldx2, const void *w_cat,
                        const kd_conv_epilogue *ep, kd_stream_t stream);

/* Workgroups of the persistent conv kernels' grids from now on: 0 = one per CU (default), else n rounded down to a multiple of 8
 * and clamped to [8, CU count] (0 < n < 8 gives 8, n above the CU count gives the full chip; the value is process-wide and atomic) -- leaves CUs to a kernel on another stream, i.e. the RCCL all-reduce of a gradient bucket that
 * parallel.GradReducer launches from inside backward (the reference's single-process trainer has no counterpart,
 * trainer/layerwise_trainer.py:235-239).  Overrides the KDCC_PERSIST_CUS environment default; results are bit-identical for any n. */
int kd_conv_set_persist_cus(int32_t n);

/* Weight packing (runs on device, on `stream`).  src: the reference's
 * nn.Conv2d.weight, fp32 (Cout, Cin, kh, kw) contiguous.
 *   KD_PACK_FWD   dst[co][ky][kx][ci]            = src[co][ci][ky][kx]
 *   KD_PACK_DGRAD dst[ci][kh-1-ky][kw-1-kx][co]  = src[co][ci][ky][kx]
 * cin_pad >= Cin (fwd) zero-fills channels [Cin, cin_pad) (decoder 304 -> 320). */
enum { KD_PACK_FWD = 0, KD_PACK_DGRAD = 1 };
int kd_pack_conv_weight(const float *src, void *dst, int32_t dtype, int32_t mode,
                        int32_t Cout, int32_t Cin, int32_t kh, int32_t kw, int32_t cin_pad,
                        kd_stream_t stream);

/* Weight gradient of a 1x1 convolution (the trainable `pointwise_conv`,
 * depthwise_separable_conv.py:9):  dw[co][ci] = sum_m dy[m][co] * a[m][ci],
 * fp32 (Cout, Cin, 1, 1) like the reference's .grad.  accumulate != 0 adds into dw
 * (gradient accumulation, layerwise_trainer.py:237-239).
 * workspace: kd_pw_wgrad_workspace() bytes. */
size_t kd_pw_wgrad_workspace(int32_t M, int32_t Cin, int32_t Cout);
int kd_pw_wgrad(int32_t dtype, int32_t M, int32_t Cin, int32_t Cout,
                const void *a, int32_t lda, const void *dy, int32_t ldy,
                float *dw, int32_t accumulate, void *workspace, size_t workspace_bytes,
                kd_stream_t stream);

/* Weight gradient of a general convolution (autograd of nn.Conv2d w.r.t. its weight, reached from loss.backward(),
 * trainer/layerwise_trainer.py:235 / trainer/classification_trainer.py:39, whenever a dense conv of the student is
 * trainable: `pruning.unfreeze` naming a dense block, models/students/depthwise_student.py:80-84, or the "identical
 * architecture" branch that unfreezes everything, layerwise_trainer.py:88-100):
 *   dw[co][ci][ky][kx] = sum_{n,ho,wo} dy[n,ho,wo,co] * x[n, ho*stride - pad + ky*dil, wo*stride - pad + kx*dil, ci]
 * fp32 (Cout, Cin, kh, kw) like the reference's .grad; d describes the forward conv (x view N,H,W,Cin with stride ldx;
 * dy view N,Ho,Wo,Cout with stride ld_dy).  One TN GEMM per tap over pixel splits, partial slabs in the workspace,
 * fixed-order reduction (deterministic).  Cin, Cout: any (multiples of 8 take the LDS-DMA path in bf16). */
size_t kd_conv2d_wgrad_workspace(const kd_conv_desc *d);
int kd_conv2d_wgrad(const kd_conv_desc *d, const void *x, const void *dy, int32_t ld_dy, float *dw,
                    int32_t accumulate, void *workspace, size_t workspace_bytes, kd_stream_t stream);

/* ------------------------------------------------------------ depthwise conv
 * `separable_conv` of depthwise_separable_conv.py:7-8: Conv2d(C, C, k,
 * padding, dilation, groups=C), stride 1 (9x9 / dilation 5 / padding 20 in
 * cfg/cityscapes/58M_deeplab_all.json:117-122; 3x3 in the CIFAR configs).
 * w_taps: [k*k][C] float (tap-major), from kd_pack_dw_weight.
 *   flip != 0 in the pack gives the dgrad operand (dx = dwconv(dy, flipped w)
 *   with pad' = dil*(k-1) - pad).
 * bias: (C) float or NULL (always NULL for the WRN-38 / ASPP targets). */
typedef struct kd_dw_desc {
    int32_t dtype;
    int32_t N, H, W, C;
    int32_t k, pad, dil;
    int32_t ldx, ldy;
} kd_dw_desc;
/* Optional epilogue (NULL = none), same meaning and order as kd_conv_epilogue's first three
 * steps; used when the kernel computes an input gradient that continues through the
 * BN(eval)+ReLU in front of the replaced conv, or accumulates into an existing gradient:
 *   v = acc; v += res_pre; v = mask > 0 ? v*mask_scale[c] : 0; v += res_post; y = v */
typedef struct kd_dw_epilogue {
    const void *res_pre;  int32_t ld_res_pre;
    const void *mask;     int32_t ld_mask;     const float *mask_scale;
    const void *res_post; int32_t ld_res_post;
} kd_dw_epilogue;
int kd_pack_dw_weight(const float *src /* (C,1,k,k) */, float *dst /* [k*k][C] */,
                      int32_t C, int32_t k, int32_t flip, kd_stream_t stream);
int kd_dwconv_fwd(const kd_dw_desc *d, const void *x, const float *w_taps, const float *bias,
                  const kd_dw_epilogue *ep, void *y, kd_stream_t stream);
/* y = sum_{i<n} dwconv(xs[i], w_taps[i]): the gradient of ONE tensor read by n depthwise convs of one geometry -- the
 * ASPP input under its replaced branches (models/deeplabv3/deeplabv3.py:64-75: every branch of `features` reads the same
 * x, so autograd sums their input gradients; with flipped tap tables and pad' as above each term is a dwconv).  All inputs
 * share d (shape, ldx); y must not alias an input.  n <= 3 bf16 9x9 inputs are summed in registers inside one launch. */
int kd_dwconv_fwd_sum(const kd_dw_desc *d, int32_t n, const void *const *xs, const float *const *w_taps, void *y,
                      kd_stream_t stream);
/* ys[i] = dwconv(x, w_taps[i]), i < n: the forward of the same fan-out (deeplabv3.py:71-75, `for f in self.features:
 * out = torch.cat((out, f(x)), 1)` with each f's 3x3 conv replaced by a DepthwiseSeparableBlock): one pass over x for up to
 * three bf16 9x9 outputs per launch.  Outputs share d->ldy and must not alias x or each other. */
int kd_dwconv_fwd_fanout(const kd_dw_desc *d, int32_t n, const void *x, const float *const *w_taps, void *const *ys,
                         kd_stream_t stream);
/* dw[c][ky][kx] = sum_{n,h,w} dy[n,h,w,c] * x[n,h-pad+ky*dil,w-pad+kx*dil,c]; fp32 (C,1,k,k). */
size_t kd_dwconv_wgrad_workspace(const kd_dw_desc *d);
int kd_dwconv_wgrad(const kd_dw_desc *d, const void *x, const void *dy, int32_t ld_dy,
                    float *dw, int32_t accumulate, void *workspace, size_t workspace_bytes,
                    kd_stream_t stream);
/* dws[i] = the weight gradient above for x and dys[i], i < n: n depthwise convs of one geometry that read ONE input -- the
 * replaced ASPP branches again (models/deeplabv3/deeplabv3.py:71-75; autograd of depthwise_separable_conv.py:7-8 per
 * branch).  For n = 2, 3 bf16 9x9 branches one launch stages each tile of x once and shares its operand windows between the
 * branches; other shapes run one kd_dwconv_wgrad per branch.  All dys share ld_dy. */
size_t kd_dwconv_wgrad_multi_workspace(const kd_dw_desc *d, int32_t n);
int kd_dwconv_wgrad_multi(const kd_dw_desc *d, int32_t n, const void *x, const void *const *dys, int32_t ld_dy,
                          float *const *dws, int32_t accumulate, void *workspace, size_t workspace_bytes,
                          kd_stream_t stream);

/* ------------------------------------------------ lattice-planar intermediates of the replaced ASPP branches
 * The depthwise outputs of the replaced branches and their gradients (models/students/transform_blocks/
 * depthwise_separable_conv.py:11-13, `x = self.separable_conv(x); x = self.pointwise_conv(x)`, under
 * models/deeplabv3/deeplabv3.py:64-75) are 4096-channel tensors that nothing but the depthwise kernels and the 1x1 convs next
 * to them ever reads.  In NHWC a depthwise workgroup (16 channels) moves them as 32-B pieces 40 KiB apart; in the
 * LATTICE-PLANAR layout of a dilation d
 *     [C/16 planes][rows][16 channels],   row(n, ry, rx, ly, lx) = ((n*d*d + ry*d + rx)*Ly + ly)*Lx + lx,
 *     Ly = ceil(H/d), Lx = ceil(W/d),  pixel (y, x) = (ry + d*ly, rx + d*lx),  rows = kd_lattice_rows() (a multiple of 256)
 * the pixels of one residue class of one image are consecutive rows, so the same tile is one contiguous run per lattice row.
 * Cells whose pixel is outside the image and the tail rows of a plane hold zeros (writers keep them zero).
 * EXPERIMENTAL / benchmark-only: no GEMM entry point of this library consumes the [C/16][rows][16] layout (the 1x1 convs next
 * to the depthwise kernels read NHWC), so nothing in the engine uses these entry points; they exist to measure what contiguous
 * depthwise intermediates are worth (1-5 %, profiles/r05_aspp_dw_lattice_ab.json) and are tested bit for bit against the NHWC
 * ones.  kd_lattice_rows_move converts between a dense [rows][C] matrix in lattice row order and image order. */
int64_t kd_lattice_rows(int32_t N, int32_t H, int32_t W, int32_t dil);
/* 1 when the fan-out / sum / multi-gradient launches of n (2 or 3) branches of geometry d can run on lattice-planar
 * intermediates (bf16, 9x9, C % 16 == 0, 32-bit plane offsets); otherwise the caller keeps NHWC intermediates. */
int32_t kd_dwconv_lattice_ok(const kd_dw_desc *d, int32_t n);
/* to_rows != 0: rows[r][c] = img[n, y, x, c] for the pixel of lattice row r (zero rows for padded cells and the tail);
 * to_rows == 0: img[n, y, x, c] = rows[r][c] for every pixel.  img: (N,H,W,C) view with pixel stride ld_img; rows:
 * kd_lattice_rows() x C with row stride ld_rows.  C and both strides multiples of 16 B. */
int kd_lattice_rows_move(int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dil, void *img, int32_t ld_img,
                         void *rows, int32_t ld_rows, int32_t to_rows, kd_stream_t stream);
/* kd_dwconv_fwd_fanout / kd_dwconv_fwd_sum / kd_dwconv_wgrad_multi with the n-side tensors lattice-planar: the fan-out's
 * outputs ys[] (x stays NHWC), the sum's inputs xs[] (y stays NHWC, stride d->ldy), the gradients dys[] (x stays NHWC).
 * n = 2 or 3; KD_ERR_UNSUPPORTED unless kd_dwconv_lattice_ok(d, n).  Same values as the NHWC entry points. */
int kd_dwconv_fwd_fanout_lattice(const kd_dw_desc *d, int32_t n, const void *x, const float *const *w_taps, void *const *ys,
                                 kd_stream_t stream);
int kd_dwconv_fwd_sum_lattice(const kd_dw_desc *d, int32_t n, const void *const *xs, const float *const *w_taps, void *y,
                              kd_stream_t stream);
int kd_dwconv_wgrad_multi_lattice(const kd_dw_desc *d, int32_t n, const void *x, const void *const *dys, float *const *dws,
                                  int32_t accumulate, void *workspace, size_t workspace_bytes /* kd_dwconv_wgrad_multi_workspace */,
                                  kd_stream_t stream);

/* ----------------------------------------------------------- trunk plumbing
 * Stem conv mod1.conv1 (wider_resnet.py:307-309): 3x3, 3 -> 64, stride 1, pad 1,
 * reading the trainer's NCHW fp32 batch directly (layerwise_trainer.py:221).
 * w: fp32 (64,3,3,3) as in the reference.  y: NHWC `dtype`, 64 channels. */
int kd_stem_conv(int32_t dtype, const float *x_nchw, const float *w, void *y,
                 int32_t N, int32_t H, int32_t W, kd_stream_t stream);
/* The same conv followed by pool2 = MaxPool2d(3, stride=2, padding=1) (wider_resnet.py:307-309, 353-356: mod1's output
 * has no other reader in DeepWV3Plus) and, for y_act, the BN(eval)+ReLU of mod2.block1 (scale/shift as in
 * kd_maxpool3x3s2), without the 64-channel full-resolution tensor ever reaching memory: for a frozen stem whose
 * output nothing else needs.  bf16 outputs (N,Ho,Wo,64), Ho = (H-1)/2+1; bit-identical to
 * kd_stem_conv(KD_BF16) + kd_maxpool3x3s2.  y_raw or y_act may be NULL. */
int kd_stem_conv_pool(const float *x_nchw, const float *w, void *y_raw, void *y_act, const float *scale,
                      const float *shift, int32_t N, int32_t H, int32_t W, kd_stream_t stream);

/* MaxPool2d(3, stride=2, padding=1) (wider_resnet.py:353-356), optionally followed
 * by the next block's BN(eval)+ReLU: y_raw (may be NULL) = pool, y_act (may be NULL) =
 * relu(pool*scale+shift). */
int kd_maxpool3x3s2(int32_t dtype, const void *x, int32_t ldx, void *y_raw, int32_t ld_raw,
                    void *y_act, int32_t ld_act, const float *scale, const float *shift,
                    int32_t N, int32_t H, int32_t W, int32_t C, kd_stream_t stream);

/* F.interpolate(bilinear, align_corners=True) (deeplabv3.py:16-18,69,155,160).
 * Input and output element types are given separately (the final logits are
 * produced in fp32 from an fp32 decoder output whatever the compute dtype). */
int kd_upsample_bilinear_ac(const void *x, int32_t x_dtype, int32_t ldx, void *y, int32_t y_dtype, int32_t ldy,
                            int32_t N, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo,
                            kd_stream_t stream);

/* The same with the align_corners flag: GSCNN's last upsample (models/gscnn/gscnn.py:323) omits align_corners, i.e.
 * src = max((o + 0.5) * I/O - 0.5, 0). */
int kd_upsample_bilinear(const void *x, int32_t x_dtype, int32_t ldx, void *y, int32_t y_dtype, int32_t ldy,
                         int32_t N, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, int32_t align_corners,
                         kd_stream_t stream);

/* ASPP image-pooling branch (deeplabv3.py:59-62,67-70): AdaptiveAvgPool2d(1) ->
 * 1x1 conv (w fp32 (Cout,Cin)) -> BN(eval) scale/shift -> ReLU -> broadcast
 * ("upsample" of a 1x1 map) into y[.., 0:Cout] of an NHWC view with stride ldy.
 * workspace: kd_aspp_image_pool_workspace() bytes (pixel-chunk partial sums, reduced in fixed order). */
size_t kd_aspp_image_pool_workspace(int32_t N, int32_t Cin, int32_t Cout);
int kd_aspp_image_pool(int32_t dtype, const void *x, int32_t ldx, const float *w, const float *scale,
                       const float *shift, void *y, int32_t ldy, int32_t N, int32_t H, int32_t W,
                       int32_t Cin, int32_t Cout, void *workspace, size_t workspace_bytes, kd_stream_t stream);
/* The same branch from per-128-pixel channel sums that the producing conv's epilogue already took (kd_conv_epilogue.bn_sums without
 * a mask: `part` = [N*H*W/128][2][Cin], rows of an image consecutive; H*W % 128 == 0): no pass over x.  Rows are added in order
 * (bit-reproducible).  Same workspace size as kd_aspp_image_pool. */
int kd_aspp_image_pool_sums(int32_t dtype, const float *part, const float *w, const float *scale, const float *shift, void *y,
                            int32_t ldy, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, void *workspace,
                            size_t workspace_bytes, kd_stream_t stream);

/* ------------------------------------------------- backward of the trunk plumbing
 * (autograd of the calls above; needed once gradients flow through the whole student: loss = kd + hint with every
 * parameter trainable, or hints taken behind a BN+ReLU such as the `aspp` module output).
 *
 * kd_stem_wgrad: weight gradient of mod1.conv1 (wider_resnet.py:307-309) from the trainer's NCHW fp32 batch:
 *   dw (64,3,3,3) fp32 = sum_pixels dy[n,h,w,:] (x) x[n,:,h-1+ky,w-1+kx].
 * kd_maxpool3x3s2_bwd: gx[n,h,w,c] = sum of gy over the (<= 4) windows whose first maximum is (h,w)
 *   (nn.MaxPool2d(3,2,1) backward, wider_resnet.py:353-356); x is the pool's input.  workspace (optional; one byte per window
 *   and channel, kd_maxpool3x3s2_bwd_workspace) selects the two-pass arg-max-index path; without it a slower gather runs.
 * kd_upsample_bilinear_ac_bwd: transpose of kd_upsample_bilinear_ac (deeplabv3.py:16-18,155,160): gy (N,Ho,Wo,C) ->
 *   gx (N,H,W,C); separable gather, workspace = one (N,Ho,W,C) float plane.
 * kd_zero_insert: y[n, h*stride, w*stride, :] = x[n,h,w,:], zeros elsewhere (Hy x Wy output): turns the input gradient
 *   of a stride-s conv (mod4.block1, wider_resnet.py:322-332) into a stride-1 kd_conv2d_fwd with KD_PACK_DGRAD weights.
 * kd_relu_bn_bwd: y = (mask > 0 ? g * scale[c] : 0) + res -- d relu(bn_eval(x))/dx applied to a gradient that arrives
 *   behind the activation (wider_resnet.py:43-48); res may be NULL.
 * kd_channel_sums: s1[b][c] = sum_m (g - sub)[m][c], s2[b][c] = sum_m (g - sub)[m][c] * a[m][c] over `groups` groups of
 *   rows_per_group consecutive rows (sub, a, s2 optional); float (groups, C); two fixed-order stages.
 * kd_bn_eval_param_grads: eval-mode BatchNorm2d weight / bias gradients from those sums of the gradient w.r.t. the BN
 *   input: dbeta = s1/scale, dgamma = (s2 - beta*s1)/(scale*gamma)   (scale = gamma/sqrt(var+eps), s2 taken against
 *   relu(bn(x)); masked elements carry zero gradient).
 * kd_broadcast_add: y[n,p,c] = (accumulate ? y : 0) + alpha * v[n,c] (backward of the ASPP image-pooling broadcast). */
size_t kd_stem_wgrad_workspace(int32_t N, int32_t H, int32_t W);
int kd_stem_wgrad(int32_t dtype, const float *x_nchw, const void *dy, int32_t ld_dy, float *dw, int32_t N, int32_t H,
                  int32_t W, int32_t accumulate, void *workspace, size_t workspace_bytes, kd_stream_t stream);
size_t kd_maxpool3x3s2_bwd_workspace(int32_t N, int32_t H, int32_t W, int32_t C);
int kd_maxpool3x3s2_bwd(int32_t dtype, const void *x, int32_t ldx, const void *gy, int32_t ldgy, void *gx, int32_t ldgx,
                        int32_t N, int32_t H, int32_t W, int32_t C, void *workspace, size_t workspace_bytes,
                        kd_stream_t stream);
size_t kd_upsample_bilinear_ac_bwd_workspace(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo);
int kd_upsample_bilinear_ac_bwd(const void *gy, int32_t gy_dtype, int32_t ldgy, void *gx, int32_t gx_dtype, int32_t ldgx,
                                int32_t N, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo,
                                void *workspace, size_t workspace_bytes, kd_stream_t stream);
/* The same transpose for either corner convention (align_corners = 0: the last upsample of GSCNN, models/gscnn/gscnn.py:323). */
int kd_upsample_bilinear_bwd(const void *gy, int32_t gy_dtype, int32_t ldgy, void *gx, int32_t gx_dtype, int32_t ldgx,
                             int32_t N, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, int32_t align_corners,
                             void *workspace, size_t workspace_bytes, kd_stream_t stream);
int kd_zero_insert(int32_t dtype, const void *x, int32_t ldx, void *y, int32_t ldy, int32_t N, int32_t H, int32_t W,
                   int32_t C, int32_t stride, int32_t Hy, int32_t Wy, kd_stream_t stream);
int kd_relu_bn_bwd(int32_t dtype, const void *g, int32_t ldg, const void *mask, int32_t ldm, const float *scale,
                   const void *res, int32_t ldres, void *y, int32_t ldy, int64_t M, int32_t C, kd_stream_t stream);
size_t kd_channel_sums_workspace(int32_t groups, int64_t rows_per_group, int32_t C);
int kd_channel_sums(int32_t dtype, const void *g, int32_t ldg, const void *sub, int32_t ldsub, const void *a, int32_t lda,
                    int32_t groups, int64_t rows_per_group, int32_t C, float *s1, float *s2,
                    void *workspace, size_t workspace_bytes, kd_stream_t stream);
int kd_bn_eval_param_grads(const float *s1, const float *s2, const float *scale, const float *gamma, const float *beta,
                           float *dgamma, float *dbeta, int32_t C, int32_t accumulate, kd_stream_t stream);
int kd_broadcast_add(int32_t dtype, const float *v, void *y, int32_t ldy, int32_t N, int64_t HW, int32_t C, float alpha,
                     int32_t accumulate, kd_stream_t stream);

/* BN(eval) scale/shift from running statistics (nn.BatchNorm2d in eval mode):
 *   scale = gamma / sqrt(var + eps),  shift = beta - mean * scale. */
int kd_bn_fold(const float *gamma, const float *beta, const float *mean, const float *var, float eps,
               float *scale, float *shift, int32_t C, kd_stream_t stream);

/* generic strided copy / cast between NCHW-or-NHWC fp32/bf16 views:
 * dst(n,c,p) = src(n,c,p), element (n,c,p) at n*sN + c*sC + p*sP (elements). */
int kd_copy_cast(const void *src, int32_t src_dtype, int64_t s_sN, int64_t s_sC, int64_t s_sP,
                 void *dst, int32_t dst_dtype, int64_t d_sN, int64_t d_sC, int64_t d_sP,
                 int32_t N, int32_t C, int64_t P, kd_stream_t stream);

/* ------------------------------------------------- small-shape path (CIFAR plumbing config)
 * NCHW fp32, the reference's own layout, for the shapes the MFMA kernels do not take: CIFAR ResNet-20
 * (models/cifar_models/resnet.py: 3/16/32/64 channels, 32x32..8x8) and the 3x3 cheap-conv blocks of the CIFAR configs
 * (depthwise_separable_conv.py:7-9 with groups = C and optional bias).
 * kd_conv2d_direct_*: nn.Conv2d forward / input gradient / weight (+ bias) gradient for any channels, kernel, stride, padding,
 *   dilation and groups.  w: (K, C/groups, kh, kw); dw like w; dbias (K) or NULL.
 * kd_bn2d_fwd / kd_bn2d_bwd: nn.BatchNorm2d forward / backward, optional fused ReLU.  training != 0: batch statistics (biased
 *   variance), save_mean / save_invstd (C) returned for the backward, running statistics updated in place with `momentum`
 *   and the unbiased variance (trainer/classification_trainer.py:21: the student runs in train mode);
 *   training == 0: the running statistics.  bwd: y (the forward output) is needed only with relu != 0; dx / dgamma / dbeta
 *   may each be NULL. */
typedef struct kd_dconv_desc {
    int32_t N, C, H, W;   /* input  (N, C, H, W) */
    int32_t K;            /* output channels */
    int32_t kh, kw, stride, pad, dil, groups;
} kd_dconv_desc;
int kd_conv2d_direct_fwd(const kd_dconv_desc *d, const float *x, const float *w, const float *bias, float *y,
                         kd_stream_t stream);
int kd_conv2d_direct_dgrad(const kd_dconv_desc *d, const float *dy, const float *w, float *dx, kd_stream_t stream);
int kd_conv2d_direct_wgrad(const kd_dconv_desc *d, const float *x, const float *dy, float *dw, float *dbias,
                           int32_t accumulate, kd_stream_t stream);
int kd_bn2d_fwd(const float *x, const float *gamma, const float *beta, float *y, float *save_mean, float *save_invstd,
                float *running_mean, float *running_var, float momentum, float eps, int32_t training, int32_t relu,
                int32_t N, int32_t C, int32_t HW, kd_stream_t stream);
int kd_bn2d_bwd(const float *dy, const float *x, const float *y, const float *gamma, const float *save_mean,
                const float *save_invstd, float *dx, float *dgamma, float *dbeta, int32_t training, int32_t relu,
                int32_t accumulate, int32_t N, int32_t C, int32_t HW, kd_stream_t stream);

/* ------------------------------------------------- BatchNorm2d on NHWC fp32 views (Wide-ResNet CIFAR path)
 * nn.BatchNorm2d between the MFMA convolutions of models/cifar_models/wrn.py (16 / 160 / 320 / 640 channels, channels-last),
 * forward and backward, train and eval mode, optional fused ReLU.  x / y / gy / res / dx are (M = N*H*W, C) fp32 views with
 * pixel strides ld* >= C (element (m, c) at base[m*ld + c]).  Any M >= 1 and C >= 1 (float4 path when C % 4 == 0 and every
 * view allows it).
 * kd_bn_nhwc_fwd, training != 0: mean[c] = (1/M) sum_m x,  var[c] = (1/M) sum_m (x - mean)^2  (biased), from per-128-pixel
 *   partials of x - k and (x - k)^2 around k = the block's first pixel, merged in a fixed order in fp64 (Chan's pairwise
 *   update) -- no fp32 E[x^2] - E[x]^2, no atomics, bit-reproducible;
 *   save_mean = mean, save_invstd = 1/sqrt(var + eps);
 *   running_mean = (1-momentum) running_mean + momentum mean,  running_var = (1-momentum) running_var + momentum var*M/(M-1)
 *   (each optional; trainer/classification_trainer.py:21 runs the student in train mode).
 *   training == 0: mean / var are the running statistics (save_mean / save_invstd written from them).
 *   y = relu?((x - mean) * gamma * invstd + beta).
 * kd_bn_nhwc_bwd: g' = relu ? g * [y > 0] : g,  xhat = (x - save_mean) * save_invstd;
 *   training: dx = gamma * invstd * (g' - mean_m(g') - xhat * mean_m(g' xhat)) (+ res);   eval: dx = gamma * invstd * g' (+ res);
 *   dbeta (+)= sum_m g',  dgamma (+)= sum_m g' xhat   (accumulate != 0: added).  res (the gradient over an identity shortcut
 *   that shares the BN's input) may be NULL; dx, dgamma, dbeta may each be NULL (frozen layers still need dx).  Same fixed-order
 *   two-stage reductions as the forward.
 * workspace: kd_bn_nhwc_workspace(M, C) bytes (train-mode forward; backward whenever a reduction is needed). */
size_t kd_bn_nhwc_workspace(int64_t M, int32_t C);
int kd_bn_nhwc_fwd(const float *x, int32_t ldx, float *y, int32_t ldy, int64_t M, int32_t C, const float *gamma, const float *beta,
                   float *save_mean, float *save_invstd, float *running_mean, float *running_var, float momentum, float eps,
                   int32_t training, int32_t relu, void *workspace, size_t workspace_bytes, kd_stream_t stream);
int kd_bn_nhwc_bwd(const float *gy, int32_t ldg, const float *x, int32_t ldx, const float *y, int32_t ldy, const float *res,
                   int32_t ldres, float *dx, int32_t lddx, int64_t M, int32_t C, const float *gamma, const float *save_mean,
                   const float *save_invstd, float *dgamma, float *dbeta, int32_t accumulate, int32_t training, int32_t relu,
                   void *workspace, size_t workspace_bytes, kd_stream_t stream);

/* ------------------------------------------------- BatchNorm2d on NHWC bf16 views (Wide-ResNet CIFAR path in bf16, csrc/bn_nhwc.hip)
 * kd_bn_nhwc_fwd / kd_bn_nhwc_bwd with x, y, gy, res and dx in bf16 storage (leading dimensions in elements); every per-channel
 * vector -- gamma, beta, the saved and running statistics, dgamma, dbeta -- stays fp32.  The semantics are the fp32 entry points',
 * flag for flag: train / eval, relu, res added to dx, dx == NULL (parameter gradients only), accumulate, the running statistics
 * updated in train mode with the unbiased variance.  dx may alias res exactly (same base and stride); no other overlap.
 * Numerics: operands are widened to fp32 on load; the statistics are the fp32 kernels' (per-128-pixel partials shifted by the
 *   block's first value, merged in fp64 with Chan's update in a fixed order, no atomics: bit-reproducible); y and dx are rounded to
 *   nearest-even once, at the store; the backward's ReLU mask is y > 0 on the stored bf16 y.
 * Vector path (8 channels = 16 B per lane) when C % 8 == 0, every base is 16-B aligned and every ld * 2 % 16 == 0; otherwise
 *   scalar (csrc/bn_select.h decides, for both storages; the kernels are the fp32 entry points', csrc/bn_nhwc_core.h, instantiated
 *   for bf16).  Any M >= 1 and C >= 1.
 * workspace: kd_bn_nhwc_lp_workspace(M, C) bytes (train-mode forward; backward whenever a reduction is needed). */
size_t kd_bn_nhwc_lp_workspace(int64_t M, int32_t C);
int kd_bn_nhwc_lp_fwd(const void *x, int32_t ldx, void *y, int32_t ldy, int64_t M, int32_t C, const float *gamma, const float *beta,
                      float *save_mean, float *save_invstd, float *running_mean, float *running_var, float momentum, float eps,
                      int32_t training, int32_t relu, void *workspace, size_t workspace_bytes, kd_stream_t stream);
int kd_bn_nhwc_lp_bwd(const void *gy, int32_t ldg, const void *x, int32_t ldx, const void *y, int32_t ldy, const void *res,
                      int32_t ldres, void *dx, int32_t lddx, int64_t M, int32_t C, const float *gamma, const float *save_mean,
                      const float *save_invstd, float *dgamma, float *dbeta, int32_t accumulate, int32_t training, int32_t relu,
                      void *workspace, size_t workspace_bytes, kd_stream_t stream);

/* ------------------------------------------------- DenseNet-BC CIFAR path (models/cifar_models/densenet.py, csrc/dense_ops.hip)
 * All fp32 on (M = N*H*W, C) views with pixel strides ld* >= C, like kd_bn_nhwc_*.
 * kd_bn_nhwc_stats: the train-mode batch statistics of kd_bn_nhwc_fwd alone -- mean, invstd = 1/sqrt(var + eps) and
 *   var_unbiased = var*M/(M-1) (var when M == 1) per channel, by the same fixed-order reduction (per channel the same bits as
 *   kd_bn_nhwc_fwd's save_mean / save_invstd on any view that holds the channel).  workspace: kd_bn_nhwc_workspace(M, C) bytes.
 * kd_bn_nhwc_apply: train-mode BatchNorm with SUPPLIED statistics, one pass: y = relu?((x - mean) * gamma * invstd + beta);
 *   running_mean = (1-momentum) running_mean + momentum mean, running_var likewise from var_unbiased, exactly as
 *   kd_bn_nhwc_fwd updates them (each optional; var_unbiased may be NULL when running_var is).  A dense block computes the
 *   statistics of each 32-channel slice of its buffer once and every later layer's norm1 applies them to its prefix.
 *   The backward is kd_bn_nhwc_bwd with mean / invstd as save_mean / save_invstd.
 * kd_avgpool2x2_nhwc / _bwd: AvgPool2d(2, 2): y (N, H/2, W/2, C), floor sizes; an odd last row / column of x is not read and
 *   its gradient is 0.  gx (N, H, W, C) is written whole.  H, W >= 2.  float4 when C % 4 == 0 and the views allow it. */
int kd_bn_nhwc_stats(const float *x, int32_t ldx, int64_t M, int32_t C, float *mean, float *invstd, float *var_unbiased, float eps,
                     void *workspace, size_t workspace_bytes, kd_stream_t stream);
int kd_bn_nhwc_apply(const float *x, int32_t ldx, float *y, int32_t ldy, int64_t M, int32_t C, const float *gamma, const float *beta,
                     const float *mean, const float *invstd, const float *var_unbiased, float *running_mean, float *running_var,
                     float momentum, int32_t relu, kd_stream_t stream);
int kd_avgpool2x2_nhwc(const float *x, int32_t ldx, float *y, int32_t ldy, int32_t N, int32_t H, int32_t W, int32_t C,
                       kd_stream_t stream);
int kd_avgpool2x2_nhwc_bwd(const float *gy, int32_t ldg, float *gx, int32_t ldgx, int32_t N, int32_t H, int32_t W, int32_t C,
                           kd_stream_t stream);

/* ------------------------------------------------- Gated-SCNN shape stream (BASELINE config 5)
 * The full-resolution pieces of models/gscnn/gscnn.py:183-325 that are not MFMA-sized convolutions.
 * kd_gated_conv: GatedSpatialConv2d.forward (models/gscnn/gate_spatial_conv.py:50-60) fused per pixel, C in {8,16,32}:
 *     u = [feat(C); gate(1)];  z = relu(W1 u + b1);  alpha = sigmoid(w2 . z + b2);  out = Wg (feat * (alpha + 1))
 *   params (fp32, contiguous): W1 [(C+1)*(C+1)], b1 [C+1], w2 [C+1], b2 [1], Wg [C*C] -- the module's two eval-mode
 *   BatchNorms folded in by the caller.  feat / out: NHWC views (ld), gate: one value per pixel (stride ldg).
 * kd_edge_attention: acts = sigmoid(cw0 * sigmoid(fuse . cs) + cw1 * canny) (gscnn.py:308-314); weights = fuse[8], cw[2].
 * kd_edge_aspp: edge branch of the ASPP module (gscnn.py:168-171): acts (N,H,W) float resampled bilinearly (align_corners)
 *   to Ho x Wo, then 1x1 conv 1 -> C (w), BN scale/shift, ReLU, written into a channel slice y (ld).
 * kd_canny: the edge map the reference gets from cv2.Canny(uint8(image), low, high) on the host (gscnn.py:284-288), on the
 *   device: Sobel 3x3 per colour channel (largest L1 magnitude wins), non-maximum suppression, hysteresis sweeps.  x: the
 *   trainer's NCHW float batch; out: (N,H,W) float 0 / 255.  `sweeps` hysteresis sweeps run; *changed (device int) ends as
 *   the number of blocks that still promoted a pixel in the last sweep: call kd_canny_continue until it reads 0.
 *   Parity of this operator is unpinned (the reference's arithmetic lives in opencv-python, not vendored). */
/* 3x3 / stride 1 / pad 1 convolution on C = 16, 32 or 64 channels, bf16 NHWC: the two convs of the shape stream's BasicBlocks res1 / res2 / res3
 * (models/encoders/Resnet.py:64-99, models/gscnn/gscnn.py:237-243) without padding them to the 64-channel GEMM granule.
 * w: bf16 [C][3][3][C] (kd_pack_conv_weight, KD_PACK_FWD; an eval-mode BatchNorm folded in by the caller), bias: fp32 (C) or NULL
 * (the folded BN shift), res: optional residual added before the ReLU (the block's identity shortcut), relu: 0 / 1.
 *   y = relu?(conv(x, w) + bias + res) */
int kd_conv3x3_small(const void *x, int32_t ldx, const void *w, const float *bias, const void *res, int32_t ldres, void *y,
                     int32_t ldy, int32_t N, int32_t H, int32_t W, int32_t C, int32_t relu, kd_stream_t stream);
/* 1x1 conv + bias on few channels, bf16 NHWC: the squeezes d1 / d2 / d3 of the shape stream (models/gscnn/gscnn.py:232-235,
 * Conv2d(64, 32, 1), Conv2d(32, 16, 1), Conv2d(16, 8, 1) at full resolution).  w: fp32 (Cout, Cin), bias: fp32 (Cout) or NULL. */
int kd_pointwise_small(const void *x, int32_t ldx, const float *w, const float *bias, void *y, int32_t ldy, int64_t npix,
                       int32_t Cin, int32_t Cout, kd_stream_t stream);
int kd_gated_conv(int32_t dtype, const void *feat, int32_t ldf, const void *gate, int32_t ldg, const float *params,
                  void *out, int32_t ldo, int64_t npix, int32_t C, kd_stream_t stream);
int kd_edge_attention(int32_t dtype, const void *cs, int32_t ldc, const float *canny, const float *weights, float *acts,
                      int64_t npix, kd_stream_t stream);
int kd_edge_aspp(int32_t dtype, const float *acts, int32_t H, int32_t W, const float *w, const float *scale,
                 const float *shift, void *y, int32_t ldy, int32_t N, int32_t Ho, int32_t Wo, int32_t C, kd_stream_t stream);
size_t kd_canny_workspace(int32_t N, int32_t H, int32_t W);
int kd_canny(const float *x, int32_t N, int32_t H, int32_t W, int32_t low, int32_t high, int32_t sweeps, float *out,
             int32_t *changed, void *workspace, size_t workspace_bytes, kd_stream_t stream);
int kd_canny_continue(int32_t N, int32_t H, int32_t W, int32_t sweeps, float *out, int32_t *changed, void *workspace,
                      size_t workspace_bytes, kd_stream_t stream);

/* -------------------------------------------------------------------- losses
 * Each writes the scalar loss (fp32, device) and, when grad != NULL, the
 * gradient w.r.t. `s` in one pass.  Views are (N, C, P) with element strides
 * (sN, sC, sP) so NCHW (reference layout) and NHWC (engine layout) are both
 * accepted; dtype per operand.  partial: workspace of kd_loss_workspace() bytes.
 *
 * kd_kldiv: KLDivergenceLoss.forward, losses/KLDiv.py:19-23
 *   loss = kl_div(log_softmax(s/T,1), softmax(t/T,1), 'mean') * T^2 * C
 *   grad = T/(N*P) * (softmax(s/T) - softmax(t/T))
 * kd_hint_mse: MSELoss.forward, losses/MSELoss.py:14-16
 *   loss = mean((s-t)^2) * num_classes ; grad = 2*num_classes*(s-t)/numel
 * kd_weighted_hint_mse: WeightedHintMSELoss.forward, losses/WeightedHintMSELoss.py:12-16
 *   w: (C) if w_per_sample == 0 else (N,C), fp32.
 * kd_ce2d: CrossEntropyLoss2d.forward, losses/CrossEntropy.py:10-14 (logged metric);
 *   target int64 (N,P), ignore_index excluded from the mean.
 */
typedef struct kd_view3 {
    const void *ptr;
    int32_t dtype;
    int64_t sN, sC, sP;
} kd_view3;
typedef struct kd_mview3 {
    void *ptr;
    int32_t dtype;
    int64_t sN, sC, sP;
} kd_mview3;

size_t kd_loss_workspace(int32_t N, int32_t C, int64_t P);
int kd_kldiv(const kd_view3 *s, const kd_view3 *t, float temperature, int32_t N, int32_t C, int64_t P,
             float *loss, const kd_mview3 *grad, float grad_scale, void *workspace, size_t workspace_bytes,
             kd_stream_t stream);
int kd_hint_mse(const kd_view3 *s, const kd_view3 *t, float num_classes, int32_t N, int32_t C, int64_t P,
                float *loss, const kd_mview3 *grad, float grad_scale, void *workspace, size_t workspace_bytes,
                kd_stream_t stream);
int kd_weighted_hint_mse(const kd_view3 *s, const kd_view3 *t, const float *w, int32_t w_per_sample,
                         int32_t N, int32_t C, int64_t P, float *loss, const kd_mview3 *grad, float grad_scale,
                         void *workspace, size_t workspace_bytes, kd_stream_t stream);
int kd_ce2d(const kd_view3 *x, const int64_t *target, int32_t ignore_index, int32_t N, int32_t C, int64_t P,
            float *loss, void *workspace, size_t workspace_bytes, kd_stream_t stream);

/* The two logged logit losses straight from the LOW-RESOLUTION logits: x_lo / s_lo / t_lo are the classifier's dense fp32
 * (N,h,w,C) NHWC outputs; the value equals kd_ce2d / kd_kldiv on F.interpolate(x, (H,W), mode='bilinear', align_corners)
 * (models/deeplabv3/deeplabv3.py:160-162 followed by losses/CrossEntropy.py:10-14 / losses/KLDiv.py:19-23), but the two
 * full-resolution fp32 tensors are never written or read: a pixel's C logits are interpolated in registers (same expression
 * tree as kd_upsample_bilinear).  Forward only (the logged metrics of trainer/layerwise_trainer.py:222-227); C <= 48 / C <= 24;
 * KD_ERR_UNSUPPORTED when the resampling ratio puts more than 160 source columns under 256 output pixels (materialise then).
 * target int64 (N,H,W); workspace as kd_loss_workspace(N, C, H*W). */
int kd_ce2d_up(const float *x_lo, const int64_t *target, int32_t ignore_index, int32_t N, int32_t h, int32_t w, int32_t C,
               int32_t H, int32_t W, int32_t align_corners, float *loss, void *workspace, size_t workspace_bytes,
               kd_stream_t stream);
int kd_kldiv_up(const float *s_lo, const float *t_lo, float temperature, int32_t N, int32_t h, int32_t w, int32_t C, int32_t H,
                int32_t W, int32_t align_corners, float *loss, void *workspace, size_t workspace_bytes, kd_stream_t stream);

/* Everything the layer-compressibility analysis logs per step (trainer/analysis_trainer.py:55-81), in ONE pass over the student's
 * and the teacher's low-resolution logits (dense fp32 (N,h,w,C), interpolated in registers as kd_ce2d_up does):
 *   out[0] = kd_ce2d(up(s), target, ignore_index)      out[1] = kd_ce2d(up(t), target, ignore_index)
 *   out[2] = mean over N*C*H*W of (up(s) - up(t))^2    (losses/MSELoss.py with reduction 'mean', num_classes 1)
 *   conf_s / conf_t: int64 (C,C) [label][prediction] of argmax_c up(s) / up(t) (first maximum), pixels whose label is outside
 *   [0, C) skipped -- kd_confusion of each tensor; accumulate != 0 adds to the matrices, else they are overwritten.
 * Forward only.  The float outputs are reduced in a fixed order (bit-reproducible), the counts are integer atomics (exact).
 * KD_ERR_UNSUPPORTED for C > 48 and for kd_ce2d_up's resampling-ratio limit: the caller then composes kd_ce2d_up / kd_hint_mse /
 * kd_confusion.  workspace as kd_loss_workspace(N, C, H*W), 8-B aligned. */
int kd_logit_metrics_up(const float *s_lo, const float *t_lo, const int64_t *target, int32_t ignore_index, int32_t N, int32_t h,
                        int32_t w, int32_t C, int32_t H, int32_t W, int32_t align_corners, float *out, int64_t *conf_s,
                        int64_t *conf_t, int32_t accumulate, void *workspace, size_t workspace_bytes, kd_stream_t stream);

/* gradient of kd_ce2d w.r.t. x (needed when the supervised loss is back-propagated: trainer/taylor_prune_trainer.py:204-206,
 * or any loss = supervised + kd + hint mix): grad[n,c,p] = grad_scale * (softmax_c(x[n,:,p]) - [c == target[n,p]]) / #valid,
 * zero for ignored pixels. */
int kd_ce2d_grad(const kd_view3 *x, const int64_t *target, int32_t ignore_index, int32_t N, int32_t C, int64_t P,
                 const kd_mview3 *grad, float grad_scale, void *workspace, size_t workspace_bytes, kd_stream_t stream);

/* CrossEntropyLoss2d(weight, size_average) (losses/CrossEntropy.py:5-14: nn.NLLLoss(weight, size_average, ignore_index) on
 * log_softmax): class_weight fp32 (C) on the device or NULL; the mean is weighted, sum_i w[y_i] nll_i / sum_i w[y_i]
 * (sum_reduction == 0, size_average=True) or the plain weighted sum (sum_reduction != 0, size_average=False); ignored
 * pixels contribute to neither.  kd_ce2d / kd_ce2d_grad are these with class_weight == NULL, sum_reduction == 0. */
int kd_ce2d_weighted(const kd_view3 *x, const int64_t *target, const float *class_weight, int32_t sum_reduction, int32_t ignore_index,
                     int32_t N, int32_t C, int64_t P, float *loss, void *workspace, size_t workspace_bytes, kd_stream_t stream);
int kd_ce2d_weighted_grad(const kd_view3 *x, const int64_t *target, const float *class_weight, int32_t sum_reduction, int32_t ignore_index,
                          int32_t N, int32_t C, int64_t P, const kd_mview3 *grad, float grad_scale, void *workspace,
                          size_t workspace_bytes, kd_stream_t stream);

/* The reference's other criteria (losses/__init__.py:2,5-7), same conventions as above; fp32 / bf16 operands, fp32 arithmetic,
 * fixed-order fp64 reductions (bit-reproducible), the loss stays on the device.  p = softmax over C, lp = log p.
 *
 * kd_jsdiv: JSDivergenceLoss.forward, losses/JSDiv.py:19-26.  ps = softmax(s/T), pt = softmax(t/T), q = (ps + pt)/2 with
 *   log q = log 1/2 + logaddexp(lps, lpt):
 *   loss = T^2/(2N) * sum_{n,c,p} [ps (lps - log q) + pt (lpt - log q)]      (divided by the batch size N only)
 *   grad = T/(2N) * ps * (a - <ps, a>_c), a = lps - log q                      (t is a constant, as in kd_kldiv)
 *   Deliberate difference: log q is evaluated as log((ps + pt)/2) -- one hardware log -- while ps + pt > 1e-30 (a normal
 *   number, where the two forms agree to a few ulp), and as log 1/2 + logaddexp(lps, lpt) below that, where ps + pt underflows.
 * kd_jsdiv_up: kd_jsdiv's forward from the two low-resolution logit tensors (see kd_kldiv_up: same limits, C <= 24).
 * kd_ensemble_kldiv: EnsembleKLDivergenceLoss.forward, losses/EnsembleKLDiv.py:17-21; t holds probabilities:
 *   loss = kl_div(log_softmax(s,1), t, 'mean') * C = 1/(N*P) * sum [xlogy(t, t) - t lps]   (0 log 0 = 0)
 *   grad = (ps * sum_c t - t) / (N*P)
 * kd_focal: FocalLoss.forward, losses/FocalLoss.py:15-28.  The inner nn.CrossEntropyLoss is already reduced (the class overwrites
 *   `reduction` after __init__, :10-12).  Per pixel, y' = y at a valid label and 0 at an ignored one (:21-22):
 *     a = (1 - p_y')^gamma at every pixel; ce = alpha_y * -lp_y at valid pixels, 0 at ignored ones; w = alpha_y at valid pixels
 *   (alpha: fp32 (C) on the device, or NULL for 1).  reduction 1 'mean': loss = mean(a) * sum ce / sum w;
 *   2 'sum': loss = sum a * sum ce; 0 'none': no scalar, a_map / ce_map (fp32 (N,P), required) hold a and ce, the caller forms
 *   the (N,N,P) product a[i] * ce[j] the reference returns.  stats (3 fp64 on the device, may be NULL): sum a, sum ce, sum w --
 *   what kd_focal_grad reads.  A label outside [0, C) that is not ignore_index counts as ignored (the reference raises).
 * kd_focal_grad: its gradient, in a second launch that reads stats and the upstream gradient on the device (no host sync):
 *   grad = u_a * da/dx + u_c * dce/dx, da/dx_c = -gamma (1-p_y')^(gamma-1) p_y' (delta_cy' - p_c), dce/dx_c = alpha_y (p_c - delta_cy)
 *   'mean': u_a = g * CE_mean / (N*P), u_c = g * mean(a) / sum w;  'sum': u_a = g * sum ce, u_c = g * sum a  (upstream: 1 fp32);
 *   'none': upstream is the dense (N,N,P) fp32 gradient G, u_a[n] = sum_j G[n,j] ce[j], u_c[n] = sum_i G[i,n] a[i] (per pixel).
 *   Deliberate difference: for gamma < 1 at p_y' == 1 (1 - p_y' rounds to 0) da/dx is 0, its limit, where the reference's autograd
 *   gives NaN (0 * inf); gamma == 0 gives da/dx = 0 everywhere.
 * kd_focal_up: kd_focal 'mean' / 'sum' from the low-resolution logits (see kd_ce2d_up: same limits, C <= 48).
 * kd_topk_hint_mse: TopkHintMSELoss.forward, losses/WeightedHintMSELoss.py:28-44, 4-D targets only.  Per sample the channels are
 *   ranked by the L2 norm of t over the P pixels and the first K kept (K = int(topk * C), computed by the caller as the reference
 *   does; 1 <= K <= C, else KD_ERR_INVALID where the reference returns NaN); num_classes is not applied:
 *   loss = sum_{n,c} mask * mean_p (s-t)^2 / (N*K) ; grad = 2 * mask * (s-t) / (P*N*K)
 *   Deliberate difference: equal norms keep the lower channel index first (the reference's argsort order is unspecified).
 *   The selection runs on the device (rank by count in LDS, C <= 4096); mask: fp32 (N,C) output or NULL.  workspace of
 *   kd_topk_hint_workspace() bytes. */
int kd_jsdiv(const kd_view3 *s, const kd_view3 *t, float temperature, int32_t N, int32_t C, int64_t P, float *loss,
             const kd_mview3 *grad, float grad_scale, void *workspace, size_t workspace_bytes, kd_stream_t stream);
int kd_jsdiv_up(const float *s_lo, const float *t_lo, float temperature, int32_t N, int32_t h, int32_t w, int32_t C, int32_t H,
                int32_t W, int32_t align_corners, float *loss, void *workspace, size_t workspace_bytes, kd_stream_t stream);
int kd_ensemble_kldiv(const kd_view3 *s, const kd_view3 *t, int32_t N, int32_t C, int64_t P, float *loss, const kd_mview3 *grad,
                      float grad_scale, void *workspace, size_t workspace_bytes, kd_stream_t stream);
int kd_focal(const kd_view3 *x, const int64_t *target, const float *alpha, float gamma, int32_t ignore_index, int32_t reduction,
             int32_t N, int32_t C, int64_t P, float *loss, double *stats, float *a_map, float *ce_map, void *workspace,
             size_t workspace_bytes, kd_stream_t stream);
int kd_focal_grad(const kd_view3 *x, const int64_t *target, const float *alpha, float gamma, int32_t ignore_index, int32_t reduction,
                  int32_t N, int32_t C, int64_t P, const double *stats, const float *upstream, const float *a_map, const float *ce_map,
                  const kd_mview3 *grad, kd_stream_t stream);
int kd_focal_up(const float *x_lo, const int64_t *target, const float *alpha, float gamma, int32_t ignore_index, int32_t reduction,
                int32_t N, int32_t h, int32_t w, int32_t C, int32_t H, int32_t W, int32_t align_corners, float *loss, double *stats,
                void *workspace, size_t workspace_bytes, kd_stream_t stream);
size_t kd_topk_hint_workspace(int32_t N, int32_t C, int64_t P);
int kd_topk_hint_mse(const kd_view3 *s, const kd_view3 *t, int32_t K, int32_t N, int32_t C, int64_t P, float *loss,
                     const kd_mview3 *grad, float grad_scale, float *mask, void *workspace, size_t workspace_bytes,
                     kd_stream_t stream);

/* The ensemble step's criterion (trainer/ensemble_trainer.py:80-85) in one pass over the student logits, and ensemble_predict
 * (:145-164).  Up to KD_MULTI_MAX operand views travel BY VALUE (`ts` is a host struct; nothing is copied to the device besides
 * the kernel arguments), each with one fp32 weight w_k >= 0; W = sum_k w_k > 0.  Operands as in kd_kldiv (fp32 / bf16, any of the
 * (N,C), NCHW, NHWC stridings, mixed freely), fp32 arithmetic, fixed-order fp64 reductions, no synchronisation.
 *
 * kd_kldiv_multi: losses[0] = kd    = (1/W) sum_k w_k * kd_kldiv(s, t_k, T)          (each KL accumulated per target)
 *                 losses[1] = sup   = kd_ce2d(s, labels, ignore_index)                (0 when labels == NULL or no pixel is valid)
 *                 losses[2] = total = kd_scale * kd + sup_scale * sup                 (three fp32 on the device)
 *   grad (when != NULL) = d total / d s
 *        = kd_scale * T/(N*P) * (softmax(s/T) - (1/W) sum_k w_k softmax(t_k/T)) + sup_scale * (softmax(s) - onehot) / #valid
 *   with a zero cross-entropy part on ignored pixels.  s and every t_k are read once where the class stride is 1 (C <= 1024: a row
 *   per wave in registers; dense NHWC with C < 22 and >= 16384 pixels: 256 pixels per block through LDS) and grad is written once;
 *   other stridings (NCHW) and larger C take one pixel per thread and re-read from cache as kd_kldiv does.  labels: int64 (N,P) or
 *   NULL.  workspace of kd_loss_workspace() bytes.  n outside [1, KD_MULTI_MAX]: KD_ERR_INVALID.
 * kd_softmax_mean: out = (1/W) sum_k w_k softmax(x_k / T, dim C), fp32, written once; out's strides are the caller's (the layout of
 *   the first view for ensemble_predict).  This is the target kd_ensemble_kldiv expects. */
#define KD_MULTI_MAX 16
typedef struct kd_multi_targets {
    int32_t n;
    kd_view3 t[KD_MULTI_MAX];
    float w[KD_MULTI_MAX];
} kd_multi_targets;
int kd_kldiv_multi(const kd_view3 *s, const kd_multi_targets *targets, float temperature, const int64_t *labels,
                   int32_t ignore_index, float kd_scale, float sup_scale, int32_t N, int32_t C, int64_t P, float *losses,
                   const kd_mview3 *grad, void *workspace, size_t workspace_bytes, kd_stream_t stream);
int kd_softmax_mean(const kd_multi_targets *logits, float temperature, int32_t N, int32_t C, int64_t P, const kd_mview3 *out,
                    kd_stream_t stream);

/* CityscapesMetricTracker.update / confusion_for_batch (utils/util.py:108-128), the logged train mIoU, without the
 * reference's two full-logit D2H copies per step (trainer/layerwise_trainer.py:249-250):
 *   for every pixel with 0 <= target < C:  conf[target][argmax_c x(n,c,p)] += 1
 * (labels == ignore_index, which the reference rewrites to C before masking, fall outside the range; argmax = first
 * index of the maximum like torch.argmax).  conf: int64 (C, C) on the device, row = label, column = prediction;
 * accumulate == 0 zeroes it first.  Integer result, exact and order-independent.  C <= 64. */
int kd_confusion(const kd_view3 *x, const int64_t *target, int32_t N, int32_t C, int64_t P,
                 int64_t *conf, int32_t accumulate, kd_stream_t stream);

/* x *= *scale with the test `*scale == 1` made on the device (then nothing is read or written): the backward of the fused
 * loss Functions, whose stored gradient is multiplied by autograd's upstream d(total)/d(loss) -- exactly 1 for
 * `loss = hint_loss` (trainer/layerwise_trainer.py:229-235).  scale: one fp32 on the device. */
int kd_scale_by_device_scalar(void *x, int32_t dtype, int64_t n, const float *scale, kd_stream_t stream);

/* ----------------------------------------------------------------- optimizer
 * RAdam.step for one tensor, utils/optim/radam.py:30-98 (fp32 params/state).
 * `step` is the per-tensor step count after the increment (radam.py:62). */
int kd_radam_step(float *p, const float *g, float *exp_avg, float *exp_avg_sq, int64_t n, int32_t step,
                  float lr, float beta1, float beta2, float eps, float weight_decay, kd_stream_t stream);
/* The same update for many tensors in one launch (mode B steps ~150 tensors): per-tensor hyper-parameters and
 * step counts, exactly the arithmetic of kd_radam_step.  `ts` is a HOST array; nothing is copied to the device besides the
 * kernel arguments. */
typedef struct kd_radam_tensor {
    float *p; const float *g; float *exp_avg; float *exp_avg_sq;
    int64_t n; int32_t step;
    float lr, beta1, beta2, eps, weight_decay;
} kd_radam_tensor;
int kd_radam_step_multi(const kd_radam_tensor *ts, int32_t count, kd_stream_t stream);

/* The steps of torch.optim.SGD, torch.optim.Adam and the reference's AdamW for many tensors in one launch (one launch per 72 /
 * 48 / 53 tensors), batched like kd_radam_step_multi: `ts` is a HOST array, per-tensor hyper-parameters and step counts, nothing
 * copied to the device besides the kernel arguments, no allocation, no sync (the call may be captured).  fp32, contiguous;
 * 16 bytes per lane where p, g and the state of a tensor are all 16-byte aligned, scalar otherwise, same value either way.
 * The scalar constants (1 - beta^step, lr / bias_correction1, sqrt(bias_correction2), the scheduled lr, 1 - dampening ...) are
 * computed here in double, as the Python of torch.optim and of the reference computes them, and rounded to float once.
 *
 * KD_OPT_SGD (torch/optim/sgd.py, _single_tensor_sgd); state[0] = momentum_buffer, touched only if momentum != 0:
 *   g = -g if MAXIMIZE;  g += weight_decay * p if weight_decay != 0
 *   if momentum != 0:  buf = g if FIRST (the buffer does not exist yet: it is written, never read)
 *                      else buf = momentum * buf + (1 - dampening) * g;   g = g + momentum * buf if NESTEROV else buf
 *   p -= lr * g
 * KD_OPT_ADAM (torch/optim/adam.py, _single_tensor_adam, not capturable); state = exp_avg, exp_avg_sq, max_exp_avg_sq (AMSGRAD):
 *   g = -g if MAXIMIZE;  g += weight_decay * p if weight_decay != 0
 *   m += (1 - beta1) * (g - m);  v = beta2 * v + (1 - beta2) * g * g;  if AMSGRAD: vmax = max(vmax, v), used in place of v
 *   p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps),   bc1 = 1 - beta1^step, bc2 = 1 - beta2^step
 * KD_OPT_ADAMW_REF (the reference's AdamW, utils/optim/radam.py:179-250); state = exp_avg, exp_avg_sq:
 *   v = beta2 * v + (1 - beta2) * g * g;  m = beta1 * m + (1 - beta1) * g
 *   slr = warmup > step ? 1e-8 + step * lr / warmup : lr
 *   p += -weight_decay * slr * p if weight_decay != 0;  p += -(slr * sqrt(bc2) / bc1) * m / (sqrt(v) + eps)
 * `step` is the per-tensor step count after the increment (unused by KD_OPT_SGD). */
enum { KD_OPT_SGD = 0, KD_OPT_ADAM = 1, KD_OPT_ADAMW_REF = 2 };
enum { KD_OPT_FIRST = 1, KD_OPT_NESTEROV = 2, KD_OPT_AMSGRAD = 4, KD_OPT_MAXIMIZE = 8 };
typedef struct kd_optim_tensor {
    float *p; const float *g; float *state[3];
    int64_t n, step;
    int32_t flags, reserved;
    double lr, weight_decay, eps, momentum, dampening, beta1, beta2, warmup;
} kd_optim_tensor;
int kd_optim_step_multi(int32_t rule, const kd_optim_tensor *ts, int32_t count, kd_stream_t stream);
/* How kd_optim_step_multi cuts its work (host side only; for tests that want a case either side of each edge): the tensors one
 * launch of `rule` holds and the elements one block steps. */
int kd_optim_launch_shape(int32_t rule, int32_t *max_tensors, int32_t *block_elems);

/* ------------------------------------------------- Gated-SCNN shape stream, backward (models/gscnn/gscnn.py:269-314 under autograd)
 * The forward kernels (kd_gated_conv, kd_pointwise_small, kd_edge_attention, kd_edge_aspp) fuse per-pixel algebra; loss.backward()
 * (trainer/layerwise_trainer.py:235) through them -- `aspp` hints, loss terms on the logits, trainable shape-stream parameters --
 * is built from these general pieces (fp32 arithmetic, either storage type, deterministic reductions):
 *
 * kd_small_linear: y[p][co] (+)= bias[co] + sum_ci w[co*Cin + ci] * x[p][ci], optional ReLU; 1 <= Cin, Cout <= 72.  The forward of any
 *   1x1 map of the stream (nn.Conv2d(C, C', 1): d1..d3, gscnn.py:232-236; the two 1x1 convs inside GatedSpatialConv2d._gate_conv,
 *   gate_spatial_conv.py:36-43) and, given the transposed matrix, its input gradient.
 * kd_small_wgrad: dw[cb*Ca + ca] = sum_p b[p][cb] * a[p][ca], db[cb] = sum_p b[p][cb] (db may be NULL): weight / bias gradient of the
 *   same maps with a = the map's input, b = the gradient of its output.
 * kd_gate_mix_bwd: GatedSpatialConv2d's tail `input_features * (alphas + 1)` (gate_spatial_conv.py:58-59) with alphas = sigmoid(a):
 *   v = feat * (sigmoid(a) + 1) (if v), gfeat = gv * (sigmoid(a) + 1) (if gfeat), ga = (sum_c gv * feat) * sigmoid'(a) (if ga).
 * kd_edge_attention_bwd: backward of kd_edge_attention (gscnn.py:308-314): g_t = dL/d(cw pre-activation), g_s = dL/d(fuse
 *   pre-activation), eo_canny[p] = (sigmoid(fuse . cs), canny) -- the cw conv's input, for its weight gradient.
 * kd_rank1_add: y[p][c] (+)= g[p] * w[c]: input gradient of a C -> 1 1x1 conv (the dsn3 / dsn4 / dsn7 side outputs, gscnn.py:272-277). */
int kd_small_linear(const void *x, int32_t x_dtype, int32_t ldx, int32_t Cin, const float *w, const float *bias, void *y,
                    int32_t y_dtype, int32_t ldy, int32_t Cout, int64_t npix, int32_t accumulate, int32_t relu,
                    const float *mask /* fp32 (npix, ldm) or NULL: y = mask > 0 ? y : 0 */, int32_t ldm, kd_stream_t stream);
size_t kd_small_wgrad_workspace(int32_t Ca, int32_t Cb, int64_t npix);
int kd_small_wgrad(const void *a, int32_t a_dtype, int32_t lda, int32_t Ca, const void *b, int32_t b_dtype, int32_t ldb, int32_t Cb,
                   int64_t npix, float *dw, float *db, int32_t accumulate, void *workspace, size_t workspace_bytes, kd_stream_t stream);
int kd_gate_mix_bwd(const void *feat, int32_t feat_dtype, int32_t ldf, const float *a, const float *gv, int32_t ldgv, float *gfeat,
                    int32_t ldgf, float *ga, float *v, int32_t ldv, int32_t C, int64_t npix, kd_stream_t stream);
int kd_edge_attention_bwd(int32_t dtype, const void *cs, int32_t ldc, const float *canny, const float *weights, const float *g_acts,
                          float *g_t, float *g_s, float *eo_canny, int64_t npix, kd_stream_t stream);
int kd_rank1_add(int32_t dtype, void *y, int32_t ldy, const float *g, const float *w, int32_t C, int64_t npix, int32_t accumulate,
                 kd_stream_t stream);

/* ----------------------------------------------------------------- diagnostics (host side only; no launch changes)
 * Kernel-selection log: the dispatchers behind kd_conv2d_fwd / kd_conv2d_wgrad / kd_pw_wgrad / kd_dwconv_* /
 * kd_stem_conv* pick one of several device kernels by shape, dtype and epilogue.  The reference has
 * nothing to mirror here -- its dispatch is cuDNN's, behind torch.nn.functional.conv2d (models/encoders/wider_resnet.py:
 * 124-167) -- but a parity test is only worth what it covers, so tests assert the kernel a case reached.
 *   kd_debug_kernel_log_enable(1) clears the counters and starts counting, (0) stops;
 *   kd_debug_kernel_log_read writes "name\tcount\n" lines (NUL-terminated, truncated to `bytes`) and returns the length
 *   needed; kd_debug_last_kernel is the name the calling thread's last dispatch picked ("" before any). */
int kd_debug_kernel_log_enable(int32_t on);
int64_t kd_debug_kernel_log_read(char *buf, size_t bytes);
const char *kd_debug_last_kernel(void);
/* The same for the plumbing dispatchers (pooling, resampling, ReLU/BN backward, channel reductions, stem, image pooling,
 * strided copy, the NCHW small-shape BatchNorm / weight gradient): the device kernel the calling thread's last such dispatch
 * picked, e.g. "channel_sums_partial_kernel<bf16,8>" ("" before any).  A slot of its own: none of these names ever enters the
 * log or kd_debug_last_kernel above.  A dispatcher that launches two kernels names the first, shape-selected one. */
const char *kd_debug_last_plumbing_kernel(void);

/* ------------------------------------------------- HRNetV2 + OCR (models/hrnet_ocr/seg_hrnet_ocr.py)
 * fp32 NHWC only; C % 4 == 0, views 16-byte aligned with ld % 4 == 0; deterministic (fixed-order reductions, no float atomics).
 *
 * kd_hr_fuse_fwd: the exchange unit of HighResolutionModule.forward (:399-414): y = relu(sum_s sample(src_s)) for 1..4 sources
 *   of C channels.  A source of the output's size is read directly; a coarser one is sampled bilinearly with
 *   align_corners=True by the coordinate rule of kd_upsample_bilinear_ac (scale 0 when an output extent is 1).  Sources are
 *   added in order.  The 1x1 conv + BN of a coarser branch and the strided 3x3 chains of a finer branch stay convolutions.
 * kd_hr_fuse_bwd: g = gy * (y > 0); gsrc[s] of the output's size receives g, a coarser one the bilinear adjoint in gather form
 *   (each source pixel sums the output pixels whose footprint touches it).  gsrc[s].ptr == NULL: that gradient is not wanted. */
typedef struct kd_hr_view {
    void *ptr;
    int32_t H, W, ld;
} kd_hr_view;
int kd_hr_fuse_fwd(const kd_hr_view *src, int32_t nsrc, void *y, int32_t ldy, int32_t N, int32_t Ho, int32_t Wo, int32_t C,
                   kd_stream_t stream);
int kd_hr_fuse_bwd(const void *gy, int32_t ldgy, const void *y, int32_t ldy, const kd_hr_view *gsrc, int32_t nsrc, int32_t N,
                   int32_t Ho, int32_t Wo, int32_t C, kd_stream_t stream);

/* SpatialGather_Module (:65-73): logits (N,HW,K) pixel stride ldl, feats (N,HW,C) pixel stride ldf, K <= 32 ->
 *   ctx (N,K,C) dense = softmax_over_HW(logits)^T . feats, and mx / lse (N,K): per class the maximum and the log-sum-exp of its
 *   logits, from which the backward recomputes the probabilities (the K x HW map is never stored).
 * kd_ocr_gather_bwd: gctx (N,K,C) and the forward's ctx, lse -> d_feats (N,HW,C), d_logits (N,HW,K); K * C * 4 <= 64 KiB.
 * workspace (both): kd_ocr_gather_workspace() bytes, 16-byte aligned. */
size_t kd_ocr_gather_workspace(int32_t N, int64_t HW, int32_t K, int32_t C);
int kd_ocr_gather_fwd(const float *logits, int32_t ldl, const float *feats, int32_t ldf, float *ctx, float *mx, float *lse, int32_t N,
                      int64_t HW, int32_t K, int32_t C, void *workspace, size_t workspace_bytes, kd_stream_t stream);
int kd_ocr_gather_bwd(const float *gctx, const float *ctx, const float *logits, int32_t ldl, const float *feats, int32_t ldf,
                      const float *lse, float *d_feats, int32_t lddf, float *d_logits, int32_t lddl, int32_t N, int64_t HW, int32_t K,
                      int32_t C, void *workspace, size_t workspace_bytes, kd_stream_t stream);

/* The core of _ObjectAttentionBlock.forward (:138-143): query (N,HW,Ck) pixel stride ldq, key / value (N,K,Ck) dense, K <= 32,
 *   2 * K * Ck * 4 <= 64 KiB -> ctx (N,HW,Ck) = softmax_K(scale * query . key^T) . value (scale = Ck^-0.5 in the reference).
 * kd_ocr_attend_bwd: g = d ctx -> d_query (N,HW,Ck), d_key, d_value (N,K,Ck); the K probabilities are recomputed per pixel;
 *   the two reductions over HW run in two fixed-order stages through `workspace` (kd_ocr_attend_workspace() bytes). */
size_t kd_ocr_attend_workspace(int32_t N, int64_t HW, int32_t K, int32_t Ck);
int kd_ocr_attend_fwd(const float *query, int32_t ldq, const float *key, const float *value, float *ctx, int32_t ldc, int32_t N, int64_t HW,
                      int32_t K, int32_t Ck, float scale, kd_stream_t stream);
int kd_ocr_attend_bwd(const float *g, int32_t ldg, const float *query, int32_t ldq, const float *key, const float *value, float *d_query,
                      int32_t lddq, float *d_key, float *d_value, int32_t N, int64_t HW, int32_t K, int32_t Ck, float scale, void *workspace,
                      size_t workspace_bytes, kd_stream_t stream);

/* ------------------------------------------------- CIFAR batches from a device-resident dataset
 * Replaces, per batch, the torchvision transform chain and the collate + H2D copy of the reference's Cifar10Dataloader /
 * Cifar100Dataloader (data_loader/data_loaders.py:13-53: RandomCrop(32, padding=4), RandomHorizontalFlip, ToTensor, Normalize,
 * one PIL image at a time with num_workers 0) by one launch.
 *   data    (n,32,32,3) uint8, pixel-interleaved; labels (n) int64: the whole dataset, resident;
 *   params  (B,4) int32 rows [index, dy, dx, flip], dy, dx in [0, 8] (4, 4, 0: the untransformed image);
 *   table   (3,256) elements of `dtype`: table[c][v] = ((v / 255) - mean[c]) / std[c], built by the caller;
 *   out     KD_CIFAR_NCHW: dense (B,3,32,32), `ld` ignored.  KD_CIFAR_NHWC: (B,32,32,ld) pixels, ld >= 3; the kernel writes the
 *           whole stride of every pixel, zeros in channels [3, ld), so `out` may come uninitialised;
 *   labels_out (B) int64 = labels[index].
 * out(b,c,y,x) = table[c][data[index_b][y + dy_b - 4][x' + dx_b - 4][c]], x' = flip_b ? 31 - x : x, and table[c][0] where that
 * pixel lies outside the image (the reference pads with 0 before ToTensor / Normalize).  No arithmetic on values: bit-identical
 * to the same composition on the host.  A row whose index, dy or dx is out of range reads nothing outside the dataset: its image
 * is all padding and its label that of the clamped index.  16-byte stores when `out` is 16-byte aligned, scalar stores otherwise;
 * B * 1024 * max(ld, 3) <= 2^31 (KD_ERR_UNSUPPORTED beyond). */
enum { KD_CIFAR_NCHW = 0, KD_CIFAR_NHWC = 1 };
int kd_cifar_batch(const uint8_t *data, const int64_t *labels, int64_t n, const int32_t *params, int32_t B, const void *table,
                   int32_t dtype, int32_t layout, void *out, int32_t ld, int64_t *labels_out, kd_stream_t stream);

/* ------------------------------------------------- Cityscapes batches from a device-resident dataset (csrc/seg_data_ops.hip)
 * Replaces, per batch, the reference's per-image chain (data_loader/cityscapes.py:179-222 with the transforms of
 * data_loader/__init__.py:7-51: RandomSizeAndCrop, RandomHorizontallyFlip, ColorJitter, RandomGaussianBlur, ToTensor, Normalize,
 * MaskToTensor; one PIL image at a time with num_workers 0) by three stages over
 *   data (n,H,W,3) uint8 and targets (n,H,W) uint8 train ids: the whole dataset, resident;
 *   params: int32 rows of `params_ld` words, one per sample, validated by the caller.  Words 0..31 are the header [index, w, h,
 *           pad_w, pad_h, x1, y1, flip, order[4], brightness, contrast, saturation (fp32 bits), hue shift byte, blur radius (0: none),
 *           jitter on, sigma (double), six Gaussian weights of offsets 0..5 (doubles)].  kd_seg_crop reads 24 S words more:
 *           HT (S,11) and VT (S,11) entries [xmin, taps <= 9, k0..k8] of PIL's bicubic passes in 22-bit fixed point for every crop
 *           column (before the flip) and row, xmin = -1 where the crop shows the pad; MX (S) and MY (S) nearest source indices of
 *           the mask, -1 for the pad.  All of it is computed on the host in double.
 * kd_seg_crop: img_out (B,S,S,3), mask_out (B,S,S) uint8 = flip(crop(pad(resize(data[index])))): the horizontal pass over the source
 *   rows a 16 x 32 tile needs, rounded and clipped to bytes, then the vertical pass, as PIL runs them (bit-identical); pad 0 / 255.
 *   A tile's windows span at most 74 source columns and 42 rows (any scale >= 0.5); a tile that asks for more, and any entry that
 *   leaves the source, reads as pad.
 * kd_seg_jitter: in place on (B,S,S,3) bytes, the four PIL operations in the row's order for every row with `jitter on`; contrast
 *   blends against int(sum(L) / (S*S) + 0.5) of the image as it stands, an exact integer sum through `workspace`
 *   (kd_seg_jitter_workspace() bytes, cleared by the call).
 * kd_seg_finish: out(b,c,y,x) = table[c][byte], byte = img[s][y][x][c] (blur 0, or a row of radius 0) or the truncated
 *   scipy.ndimage.gaussian_filter of img / 255. in double with the row's weights (blur 1; radius <= 5, edges replicated);
 *   s = index_b (use_index 1: img is the dataset, n images) or b (img is a batch of n >= B images); mask_out (B,H,W) int64.
 *   table (3,256) elements of `dtype`.  KD_SEG_NCHW: dense (B,3,H,W), `ld` ignored.  KD_SEG_NHWC: (B,H,W,ld) pixels, ld >= 3; the
 *   kernel writes every pixel's whole stride, zeros in channels [3, ld).  16-byte stores when out and mask_out are 16-byte aligned
 *   and a row of W (NCHW) or W * ld (NHWC) elements is whole 16-byte pieces, scalar stores otherwise.
 * H, W, S <= 32768 and B <= 65535 (KD_ERR_UNSUPPORTED beyond). */
enum { KD_SEG_NCHW = 0, KD_SEG_NHWC = 1 };
int kd_seg_crop(const uint8_t *data, const uint8_t *targets, int64_t n, int32_t H, int32_t W, const int32_t *params, int64_t params_ld, int32_t B,
                int32_t S, uint8_t *img_out, uint8_t *mask_out, kd_stream_t stream);
size_t kd_seg_jitter_workspace(int32_t B);
int kd_seg_jitter(uint8_t *img, const int32_t *params, int64_t params_ld, int32_t B, int32_t S, void *workspace, size_t workspace_bytes,
                  kd_stream_t stream);
int kd_seg_finish(const uint8_t *img, const uint8_t *mask, int64_t n, int32_t H, int32_t W, const int32_t *params, int64_t params_ld, int32_t B,
                  int32_t use_index, int32_t blur, const void *table, int32_t dtype, int32_t layout, void *out, int32_t ld, int64_t *mask_out,
                  kd_stream_t stream);

/* ------------------------------------------------- per-tile class statistics of the resident label maps (csrc/seg_stats_ops.hip)
 * Replaces the centroid pass of the reference's class-uniform sampling (data_loader/uniform.py:47-108: per image a PIL decode, a
 * 34-pass id remap and scipy.ndimage.center_of_mass per tile and class on a thread pool, cached in a JSON file) by one pass over
 *   targets (n,H,W) uint8 train ids, the resident label maps;
 *   stats   (n, H / tile, W / tile, num_classes, 3) int64 = [count, sum of x, sum of y] of the pixels of class c inside the tile,
 *           x and y relative to the tile's origin.  Tiles are tile x tile in row-major order; remainder rows and columns belong to
 *           no tile; label 255 and any value >= num_classes count nowhere.  The call clears `stats` itself.  The reference's
 *           centroid of a tile and class is (x_offs + sum_x / count, y_offs + sum_y / count) in integer division.
 * Exact integer sums: per-workgroup uint32 partials in LDS, then one 64-bit atomic add per non-zero partial, so the result is the
 * same bits whatever the order and from run to run.  16-byte loads when targets is 16-byte aligned and W and tile are multiples of
 * 16, byte loads otherwise (csrc/seg_stats_select.h decides).  H < tile or W < tile: nothing to write, KD_OK without a launch.
 * H, W <= 32768 and 1 <= num_classes <= 64 (KD_ERR_UNSUPPORTED beyond); tile >= 1 and n >= 1 (KD_ERR_INVALID). */
int kd_seg_class_stats(const uint8_t *targets, int64_t n, int32_t H, int32_t W, int32_t tile, int32_t num_classes, int64_t *stats,
                       kd_stream_t stream);

/* ------------------------------------------------- classifier head of the CIFAR pre-activation ResNet (csrc/head_ops.hip)
 * The reference's PreResNet ends in bn -> relu -> AvgPool2d(8) on an 8x8 map (models/cifar_models/preresnet.py:150-153).  One pass
 * that never stores the activation:
 *   pooled[n][c] = (1/HW) sum_p max((x[n][p][c] - mean[c]) invstd[c] gamma[c] + beta[c], 0)
 *   x       fp32 NHWC view, pixel (n, p) at x + (n HW + p) ldx, ldx >= C;  pooled dense (N,C);
 *   gamma, beta, mean, invstd  (C) fp32: eval mode passes the running mean and 1/sqrt(running_var + eps), train mode what
 *           kd_bn_nhwc_stats gave.  running_mean / running_var (each may be NULL) are then updated in place as kd_bn_nhwc_apply does,
 *           running <- (1 - momentum) running + momentum v, from mean and var_unbiased (needed with running_var only).
 * The backward recomputes the activation's sign from x.  With g'[n][p][c] = gpooled[n][c] / HW where the activation is positive and
 * 0 elsewhere, and xhat = (x - mean) invstd, M = N HW:
 *   dbeta = sum g',  dgamma = sum g' xhat,
 *   dx = gamma invstd (g' - dbeta / M - xhat dgamma / M) in train mode, gamma invstd g' in eval mode; pixel stride lddx >= C.
 *   dx may be NULL (then lddx is ignored); dgamma and dbeta are always written.
 * A workgroup owns four channels over all N HW pixels: no workspace, no atomics, fixed-order sums (the same bits every run), correct
 * at any size and meant for CIFAR's (a few MB).  16-byte accesses when C % 4 == 0 and x and dx (when given) are 16-byte aligned with
 * pixel strides that are multiples of 4, scalar accesses otherwise (csrc/head_select.h decides). */
int kd_head_bn_relu_pool_fwd(const float *x, int32_t ldx, int32_t N, int32_t HW, int32_t C, const float *gamma, const float *beta,
                             const float *mean, const float *invstd, float *pooled, const float *var_unbiased, float *running_mean,
                             float *running_var, float momentum, kd_stream_t stream);
int kd_head_bn_relu_pool_bwd(const float *x, int32_t ldx, const float *gpooled, int32_t N, int32_t HW, int32_t C, const float *gamma,
                             const float *beta, const float *mean, const float *invstd, float *dx, int32_t lddx, float *dgamma,
                             float *dbeta, int32_t training, kd_stream_t stream);

/* ------------------------------------------------- dropout (csrc/dropout.hip; the rule: csrc/dropout_rng.h)
 * y[m][c] = keep(m, c) ? x[m][c] * scale : 0 for an (M, C) NHWC view, dtype KD_F32 or KD_BF16 (the product in fp32, bf16 rounded to
 * nearest-even once, at the store); ldx, ldy >= C are the pixel strides in elements.  The mask is a pure function of
 * (seed, offset, idx) and of nothing else -- layout, strides, dtype, vector width and grid do not change it:
 *   idx = m * C + c as int64, m the pixel index (n*H + h)*W + w, c the logical channel, C the logical channel count;
 *   Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key increments 0x9E3779B9 / 0xBB67AE85, 10 rounds) with
 *   key = (seed & 0xffffffff, seed >> 32), counter = (q & 0xffffffff, q >> 32, offset & 0xffffffff, offset >> 32), q = idx >> 2;
 *   element idx uses output word idx & 3 and is kept iff word >= threshold.
 * The caller turns a rate p into threshold = floor(p * 2^32) and scale = 1 / (1 - p).  The same call with the forward's
 * (seed, offset) is the backward: dx = dropout(gy); nothing is stored between the two.  x == y is allowed (a thread loads its
 * elements before it stores them and touches no others); channels [C, ld) of a padded view are neither read nor written.  No
 * workspace.  A lane takes 16 bytes (4 fp32 or 8 bf16 channels) when C is a multiple of that and both views are 16-byte aligned with
 * 16-byte-multiple pixel strides, one Philox block of scalar accesses otherwise (csrc/dropout_select.h decides). */
int kd_dropout_nhwc(const void *x, int32_t ldx, void *y, int32_t ldy, int32_t dtype, int64_t M, int32_t C, uint32_t threshold, float scale,
                    uint64_t seed, uint64_t offset, kd_stream_t stream);

/* ------------------------------------------------- BatchNorm -> ReLU -> MaxPool2d(2, 2) of the CIFAR VGGs (csrc/pool_ops.hip)
 * The reference's VGG `features` hold conv, BatchNorm2d, ReLU, MaxPool2d(kernel_size=2, stride=2) five times
 * (models/cifar_models/vgg.py:53-66).  One pass that reads x once and never stores the full-resolution activation:
 *   y[n][ho][wo][c] = max over ky, kx in {0, 1} of max((x[n][2 ho + ky][2 wo + kx][c] - mean[c]) (gamma[c] invstd[c]) + beta[c], 0)
 *   x       fp32 NHWC view (N,H,W,C), pixel stride ldx >= C;  y (N,H/2,W/2,C), pixel stride ldy >= C; H, W >= 2 (KD_ERR_INVALID
 *           otherwise); an odd last row or column is dropped, as nn.MaxPool2d does.
 *   gamma, beta, mean, invstd  (C) fp32, or all four NULL for the form without BatchNorm, y = max over the window of max(x, 0).  Eval
 *           mode passes the running mean and 1/sqrt(running_var + eps), train mode what kd_bn_nhwc_stats gave; running_mean /
 *           running_var (each may be NULL) are then updated in place as kd_bn_nhwc_apply does,
 *           running <- (1 - momentum) running + momentum v, from mean and var_unbiased (needed with running_var only).
 * The backward saves nothing: it recomputes the four activations of every window from x.  g' is gpooled[n][ho][wo][c] (pixel stride
 * ldg >= C) at the FIRST position in (ky, kx) order that holds the window's maximum, where that maximum is positive, and 0 at every
 * other pixel: MaxPool2d's backward followed by ReLU's.  With xhat = (x - mean) invstd and M = N H W (every pixel counts, those of a
 * dropped row or column too):
 *   dbeta = sum g',  dgamma = sum g' xhat,
 *   dx = gamma invstd (g' - dbeta / M - xhat dgamma / M) in train mode, gamma invstd g' in eval mode, g' without BatchNorm (then
 *   dgamma and dbeta are NULL and dx is required); pixel stride lddx >= C.  With BatchNorm dx may be NULL (lddx is then ignored) and
 *   dgamma and dbeta are always written.
 * The sums are two fixed-order stages and no atomics (the same bits every run); with BatchNorm the backward needs
 * kd_bn_nhwc_workspace(N H W, C) bytes of workspace (it uses less), without it none.  16-byte accesses when C % 4 == 0 and every
 * activation view of the call is 16-byte aligned with a pixel stride that is a multiple of 4, scalar accesses otherwise
 * (csrc/pool_select.h decides). */
int kd_bn_relu_maxpool2x2_fwd(const float *x, int32_t ldx, int32_t N, int32_t H, int32_t W, int32_t C, const float *gamma, const float *beta,
                              const float *mean, const float *invstd, float *y, int32_t ldy, const float *var_unbiased, float *running_mean,
                              float *running_var, float momentum, kd_stream_t stream);
int kd_bn_relu_maxpool2x2_bwd(const float *x, int32_t ldx, const float *gpooled, int32_t ldg, int32_t N, int32_t H, int32_t W, int32_t C,
                              const float *gamma, const float *beta, const float *mean, const float *invstd, float *dx, int32_t lddx,
                              float *dgamma, float *dbeta, int32_t training, void *workspace, size_t workspace_bytes, kd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KDCC_H */
