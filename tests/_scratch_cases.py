"""The rows of tests/test_scratch_gpu.py: which existing GPU test, on which row of its table, is run again with poisoned, guarded
scratch memory (tests/_scratch.py).  Nothing here touches the device: tests/test_scratch_host.py holds the table against
include/kdcc.h (every kd_*_workspace export has a row) and against the case tables it points into.

A row names
  sizing   the kd_*_workspace functions whose bytes the entry point hands the library in this row,
  module   the GPU test module and `test` the function in it that builds the row's inputs, launches, asserts the kernel the table
           names and holds the result to the table's reference and bound (run once per fill, unchanged),
  entries  the ops functions whose operands and results are recorded and compared between the fills,
  table    the case-table module whose CASES holds the dict with id `case` (passed as the test's `c`), or
  args     the test's other parameters (the tables of tuples: _dw_dispatch_cases, test_bn_lp_gpu.SHAPES).
Rows are the smallest of each kernel that reads or writes scratch, plus the rows their tables comment as ragged: a last chunk
shorter than the others, fewer blocks than slots, a 1-row tile, staged finishers, launches that share one workspace, all-ignored
criteria.  No tensor of a row is over 32 MiB.
"""
import _dw_dispatch_cases as D

ROWS = []


def row(sizing, module, test, entries, table=None, case=None, **args):
    sizing = (sizing,) if isinstance(sizing, str) else tuple(sizing)
    entries = (entries,) if isinstance(entries, str) else tuple(entries)
    tag = case if case is not None else "-".join(str(v).replace(" ", "") for v in args.values())
    r = dict(id=f"{test.replace('test_', '')}|{tag}" if tag else test.replace("test_", ""), sizing=sizing, module=module, test=test, entries=entries,
             table=table, case=case, args=args)
    ROWS.append(r)
    return r


def rows(sizing, module, test, entries, table, cases):
    for c in cases:
        row(sizing, module, test, entries, table, c)


# ------------------------------------------------------------------------------------------ trunk / backward plumbing (bwd_ops.hip)
PL = ("test_plumbing_gpu", "_plumbing_cases")
rows("kd_channel_sums_workspace", PL[0], "test_channel_sums", "channel_sums", PL[1], [
    "channel_sums:lc4-one-chunk-f32", "channel_sums:lc4-one-chunk-bf16",      # one chunk: the smallest
    "channel_sums:ragged-cblock-f32",                                         # a channel block of one vector
    "channel_sums:vec1-C19-bf16", "channel_sums:vec1-C3-f32",                 # C % 8 != 0: the scalar kernel; fewer channels than lanes
    "channel_sums:chunks-ragged-f32", "channel_sums:chunks-ragged-bf16",      # 137 chunks of 511 rows, the last 504
    "channel_sums:want-clamp-16-per-image-bf16",                              # 16 chunks where cs_chunks is 17, per image, last chunk 505
    "channel_sums:per-image-ragged-f32",
    "channel_sums:cap-1024-f32", "channel_sums:cap-1024-bf16"])               # the 1024-chunk cap, ragged last chunk
rows("kd_bn_sums_finish_workspace", PL[0], "test_bn_sums_finish", "bn_sums_finish", PL[1], [
    "bn_sums_finish:rows1-C8", "bn_sums_finish:rows256-C24",                  # one kernel, no stage
    "bn_sums_finish:rows257-C8", "bn_sums_finish:rows1000-C24",               # staged: 64-row stages, 1000 = 15 * 64 + 40
    "bn_sums_finish:rows16384-C8", "bn_sums_finish:rows16385-C24"])           # 256 full stages; 256-row stages with a 1-row last one
rows("kd_aspp_image_pool_workspace", PL[0], "test_aspp_image_pool", "aspp_image_pool", PL[1], [
    "aspp_image_pool:6x10-empty-chunks-f32", "aspp_image_pool:6x10-empty-chunks-bf16",      # 60 pixels under 64 chunks: four empty ones
    "aspp_image_pool:37x41-cin264-f32", "aspp_image_pool:37x41-cin264-bf16"])
rows("kd_stem_wgrad_workspace", PL[0], "test_stem_wgrad", "stem_wgrad", PL[1], [
    "stem_wgrad:valu-off1", "stem_wgrad:mfma-dense", "stem_wgrad:f32-dense", "stem_wgrad:mfma-800-items", "stem_wgrad:valu-800-items"])
rows("kd_maxpool3x3s2_bwd_workspace", PL[0], "test_maxpool_bwd", "maxpool3x3s2_bwd", PL[1], [
    "maxpool_bwd:argmax-1x1-f32", "maxpool_bwd:argmax-13x18-bf16", "maxpool_bwd:argmax-64x13-f32", "maxpool_bwd:argmax-C264-bf16",
    "maxpool_bwd:scalar-C19-f32"])                                            # a workspace handed to the kernel that has no use for it
rows("kd_upsample_bilinear_ac_bwd_workspace", PL[0], "test_upsample_bwd", "upsample_bilinear_ac_bwd", PL[1], [
    "upsample_bwd:v8-f32-f32-ac-6x9to12x18", "upsample_bwd:v1-bf16-f32-ac-32x48to4x6", "upsample_bwd:v1-f32-bf16-nac-7x10to18x23",
    "upsample_bwd:v8-bf16-bf16-nac-5x7to9x1", "upsample_bwd:v8-C256-bf16-bf16-ac"])

# --------------------------------------------------------------------------------- conv weight gradients and epilogue sums (pw_wgrad.hip)
CV = ("test_conv_dispatch_gpu", "_conv_dispatch_cases")
# (test_weight_gradient_gate hands `workspace=` a buffer of its own, of exactly the ABI's bound, which would pass the seam by: the
# recorder of test_scratch_gpu.py replaces it with None, so ops.py allocates the same `need` bytes at the seam.  These rows therefore
# check the scratch, not the caller-supplied-buffer path; that stays the business of test_conv_dispatch_gpu.py itself.)
rows("kd_conv2d_wgrad_workspace", CV[0], "test_weight_gradient_gate", "conv2d_wgrad", CV[1], [
    "wgrad:plan.one_stage.row", "wgrad:row.cout128",        # conv_wgrad_lw_kernel: one stage; several
    "wgrad:row.cout136",                                    # conv_wgrad_row_kernel, ragged second Cout tile
    "wgrad:plan.one_stage", "wgrad:plan.under4", "wgrad:row.w72",       # pw_wgrad_tr_kernel: one split
    "wgrad:wide.cin248",                                    # two ragged Cin tiles
    "wgrad:wide.cin256", "wgrad:wide.m%64",                 # conv_wgrad_pw_lw_kernel; conv_wgrad_wide_kernel with a masked last stage
    "wgrad:gen.cout19", "wgrad:row.f32"])                   # the generic kernels: a reduce that is no multiple of 4
rows("kd_pw_wgrad_workspace", CV[0], "test_weight_gradient_gate", "pw_wgrad", CV[1], ["pw:tr", "pw:cin256", "pw:m%64", "pw:inside135"])
rows("kd_bn_sums_finish_workspace", CV[0], "test_forward_gate", "conv2d", CV[1], [
    "fwd:pp128.sums.mask", "fwd:pp128.sums.mask.h=dil"])    # `part`: the epilogue's eval-BN partial rows and their finisher
# `opart`, the output sums of the ping-pong 1x1 kernel (the table's fwd:out_sums row), and aspp_image_pool(sums=) on them
row("kd_aspp_image_pool_workspace", "test_scratch_gpu", "run_image_pool_from_sums", ("conv2d", "aspp_image_pool"))

# ------------------------------------------------------------------------------------------- depthwise weight gradients (dwconv*.hip)
TO = "test_ops_gpu"
for _dt, _case in (("bf16", D.DW_CASES[1]), ("f32", D.DW_CASES[1]), ("bf16", D.DW_CASES[0]), ("bf16", D.DW_CASES[2])):
    row("kd_dwconv_wgrad_workspace", "test_scratch_gpu", "run_dwconv_wgrad", "dwconv_wgrad", dt=_dt, shape=_case)
for _dt, _i in (("bf16", 0),        # the smallest: one half-height tile pair per class
                ("bf16", 4),        # 14 lattice rows: a 13-row and a 1-row tile
                ("bf16", 5),        # C % 16 != 0: one register-kernel launch per branch, one workspace
                ("bf16", 6),        # four branches: three fused + one single, one workspace
                ("f32", 6), ("bf16", 7), ("f32", 0)):
    row("kd_dwconv_wgrad_multi_workspace", TO, "test_dwconv_wgrad_multi", "dwconv_wgrad_multi", dt=_dt, shape=D.WGRAD_MULTI_CASES[_i])
for _i in (0, 3):
    row("kd_dwconv_wgrad_multi_workspace", TO, "test_dwconv_wgrad_multi_lattice", ("dwconv_wgrad_multi_lattice", "dwconv_wgrad_multi"),
        shape=D.LATTICE_CASES[_i])
# (no rows: the "ONE work item per workgroup" rows of LONE_WAVE_CASES are forward fan-outs, dw_lw_fan3_kernel, and the "more inputs
# than one launch sums" row of SUM_CASES is kd_dwconv_fwd_sum, which chains its launches through its output: neither takes scratch,
# and a row that is handed no buffer fails as vacuous.  The launches that do share one workspace inside a call are the
# four-branch weight gradients above.)

# --------------------------------------------------------------------------------------------------- NHWC BatchNorm, fp32 and bf16
NH = ("test_nhwc_support_gpu", "_nhwc_support_cases")
rows("kd_bn_nhwc_workspace", NH[0], "test_bn_nhwc_fwd", "bn_nhwc_fwd", NH[1], [
    "bn_fwd:M1-C1-train-relu1", "bn_fwd:M384-C4-train-relu1", "bn_fwd:M2048-C6-train-relu0", "bn_fwd:M2049-C17-train-relu0",
    "bn_fwd:M129-C65-train-relu1"])
rows("kd_bn_nhwc_workspace", NH[0], "test_bn_nhwc_bwd", "bn_nhwc_bwd", NH[1], [
    "bn_bwd:M1-C1-train-relu1", "bn_bwd:M384-C4-train-relu1",                 # 3 and 1 empty row blocks in the backward's partials
    "bn_bwd:M2048-C6-train-relu0", "bn_bwd:M2049-C17-train-relu0",            # 16 row blocks, one finisher trip; 17, two
    "bn_bwd:M513-C4-eval-relu0", "bn_bwd:no-dx-dgamma-only", "bn_bwd:accumulate", "bn_bwd:accumulate-scalar"])
rows("kd_bn_nhwc_workspace", NH[0], "test_bn_nhwc_stats", ("bn_nhwc_stats", "bn_nhwc_fwd"), NH[1], [
    "bn_stats:M1-C17", "bn_stats:M129-C17", "bn_stats:M2049-C17", "bn_stats:M513-C8-slice"])
LP = "test_bn_lp_gpu"
for _shape in ((1, 6, None), (129, 8, None), (2049, 160, None), (2049, 64, (0, 65))):
    row("kd_bn_nhwc_lp_workspace", LP, "test_forward", "bn_nhwc_fwd", shape=_shape, train=True, relu=True)
    row("kd_bn_nhwc_lp_workspace", LP, "test_backward", "bn_nhwc_bwd", shape=_shape, train=True, relu=True, with_res=_shape[0] == 129)
row("kd_bn_nhwc_lp_workspace", LP, "test_backward", "bn_nhwc_bwd", shape=(2048, 64, (8, 72)), train=False, relu=False, with_res=True)
row("kd_bn_nhwc_lp_workspace", LP, "test_backward_accumulate", "bn_nhwc_bwd", layout=(6, None))
row("kd_bn_nhwc_lp_workspace", LP, "test_backward_accumulate", "bn_nhwc_bwd", layout=(160, None))

# ------------------------------------------------------------------------------------------------------------- OCR (hrnet_ops.hip)
rows("kd_ocr_gather_workspace", NH[0], "test_ocr_gather", "ocr_gather", NH[1], [
    "ocr_gather:min-1px-1class", "ocr_gather:two-chunks-second-1px", "ocr_gather:hw2113-two-tiles", "ocr_gather:hw8257-two-stats-trips",
    "ocr_gather:views"])
rows("kd_ocr_gather_workspace", NH[0], "test_ocr_gather_bwd", "ocr_gather_bwd", NH[1], [
    "ocr_gather_bwd:min-1px-1class", "ocr_gather_bwd:two-chunks-second-1px", "ocr_gather_bwd:hw1025-ppb16", "ocr_gather_bwd:hw2113-two-tiles"])
rows("kd_ocr_attend_workspace", NH[0], "test_ocr_attend_bwd", "ocr_attend_bwd", NH[1], [
    "ocr_attend_bwd:min", "ocr_attend_bwd:K2", "ocr_attend_bwd:hw1025-four-trips", "ocr_attend_bwd:hw2113-two-tiles", "ocr_attend_bwd:views"])

# ---------------------------------------------------------------------------------------------------- shape stream (gscnn_*.hip)
SS = ("test_shape_stream_gpu", "_shape_stream_cases")
rows("kd_small_wgrad_workspace", SS[0], "test_small_wgrad", "small_wgrad", SS[1], [
    "small_wgrad:33x33-n1", "small_wgrad:33x33-n65-bf16", "small_wgrad:2x1-n1479", "small_wgrad:72x72-n4097", "small_wgrad:33x33-n8300",
    "small_wgrad:33x33-n4097-slices", "small_wgrad:33x33-n4097-acc", "small_wgrad:72x72-n4097-acc-nobias", "small_wgrad:17x17-n65-acc-bf16"])
# (ops.canny allocates once: kd_canny finds the poison, kd_canny_continue what kd_canny left -- the pair must equal the clean pair)
rows("kd_canny_workspace", SS[0], "test_canny_reaches_the_hysteresis_fixed_point", "canny", SS[1], [
    "canny:noise-1x1", "canny:noise-3x5", "canny:line-seed-right"])

# ---------------------------------------------------------------------------------------------------------- criteria (losses.hip)
LS = ("test_loss_dispatch_gpu", "_loss_dispatch_cases")
LOSS_ENTRIES = ("kldiv", "jsdiv", "ensemble_kldiv", "hint_mse", "weighted_hint_mse", "topk_hint_mse", "ce2d", "ce2d_grad", "ce2d_up", "kldiv_up",
                "jsdiv_up", "focal_up", "logit_metrics_up", "focal", "focal_grad", "kldiv_multi")
_first_loss = len(ROWS)
rows("kd_loss_workspace", LS[0], "test_pair", LOSS_ENTRIES, LS[1], [
    "pair:kld-nhwc-f32-f32-f32", "pair:kld-nchw", "pair:kld-2d", "pair:kld-C33", "pair:kld-nograd", "pair:kld-cslice-g",
    "pair:jsd-nhwc-bf16-bf16-bf16", "pair:jsd-nchw", "pair:jsd-underflow", "pair:ekl-nhwc-f32-f32-f32", "pair:ekl-nchw-bf16", "pair:ekl-zeros"])
rows("kd_loss_workspace", LS[0], "test_hint_mse", LOSS_ENTRIES, LS[1], [
    "hint_mse:vec-cl-f32", "hint_mse:numel-rem4-f32", "hint_mse:vec-cl-bf16", "hint_mse:off1-f32", "hint_mse:nograd"])
rows("kd_loss_workspace", LS[0], "test_weighted_hint_mse", LOSS_ENTRIES, LS[1], [
    "whmse:P30-shared", "whmse:P65-per-sample", "whmse:P4097-shared", "whmse:C260-two-channel-blocks"])
rows("kd_topk_hint_workspace", LS[0], "test_topk_hint_mse", LOSS_ENTRIES, LS[1], [
    "topk:cfast-C24-f32", "topk:cfast-C20-f32", "topk:pfast-P40-f32", "topk:pfast-P36-bf16", "topk:nograd", "topk:k1",
    "topk:C70-two-channel-groups"])
rows("kd_loss_workspace", LS[0], "test_ce2d", LOSS_ENTRIES, LS[1], [
    "ce2d:nhwc-f32", "ce2d:nchw-f32", "ce2d:C65", "ce2d:2d", "ce2d:all-ignored-cl", "ce2d:all-ignored-nchw"])
rows("kd_loss_workspace", LS[0], "test_ce2d_grad", LOSS_ENTRIES, LS[1], [
    "ce2d_grad:plain-cl", "ce2d_grad:plain-nchw", "ce2d_grad:plain-cs", "ce2d_grad:weighted", "ce2d_grad:all-ignored"])
rows("kd_loss_workspace", LS[0], "test_up", LOSS_ENTRIES, LS[1], [
    "ce2d_up:C18-ac", "ce2d_up:C19-ac", "ce2d_up:W257-ac", "ce2d_up:all-ignored-ac", "kldiv_up:C19-ac", "kldiv_up:C20-hp", "jsdiv_up:C19-ac",
    "focal_up:C19-ac", "metrics_up:C19-ac", "metrics_up:all-ignored-ac"])
rows("kd_loss_workspace", LS[0], "test_focal", LOSS_ENTRIES, LS[1], ["focal:mean-cl", "focal:none-nchw", "focal:bf16", "focal_grad:mean-cl"])
rows("kd_loss_workspace", LS[0], "test_kldiv_multi_and_softmax_mean", LOSS_ENTRIES, LS[1], [
    "kldiv_multi:C100-vec", "kldiv_multi:C260", "kldiv_multi:C1028", "kldiv_multi:nchw-any", "kldiv_multi:cl-wave", "kldiv_multi:C19-rows16384",
    "kldiv_multi:nograd"])
CRITERION_ROWS = ROWS[_first_loss:]        # in table order: the two sequence tests run them through one shared cache buffer

# ------------------------------------------------------------------------------------------------- colour jitter (seg_data_ops.hip)
row("kd_seg_jitter_workspace", "test_cityscapes_loader_gpu", "test_the_jitter_kernels_equal_the_host_path_for_every_operation_and_order_class",
    "seg_jitter")


def ids(rs=ROWS):
    return [r["id"] for r in rs]


def sizing_covered():
    return {s for r in ROWS for s in r["sizing"]}
