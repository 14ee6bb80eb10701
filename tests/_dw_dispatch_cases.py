"""The depthwise dispatch cases and the rule that predicts which kernel each runs on: shared by tests/test_ops_gpu.py (which launches
every row on the GPU and asserts the kernel log) and tests/test_dw_select_host.py (which holds csrc/dw_select.h against the same rule
without a GPU).  The tensors of these rows are dense and allocator-aligned, so the rule reads the shape and the dtype alone."""

# N, H, W, C, k, pad, dil
DW_CASES = [(2, 24, 32, 16, 9, 20, 5), (1, 8, 8, 16, 3, 1, 1), (1, 23, 37, 72, 9, 20, 5), (2, 6, 50, 8, 9, 20, 5),
            # matrix-core path (bf16, C % 16 == 0): several lattice tiles with real halos, dil 1, ragged last tiles
            (1, 140, 270, 32, 9, 20, 5), (1, 40, 70, 16, 9, 4, 1), (2, 64, 128, 48, 9, 20, 5)]

SUM_CASES = [
    # N, H, W, C, k, pad, dil, inputs
    (2, 24, 32, 16, 9, 20, 5, 3),        # one lattice tile per residue class (the ASPP shape in small)
    (1, 140, 270, 32, 9, 20, 5, 3),      # several tiles with real halos, ragged last tiles
    (1, 40, 70, 16, 9, 4, 1, 2),         # two inputs, dil 1
    (2, 64, 128, 48, 9, 20, 5, 3),       # three channel groups
    (1, 23, 37, 72, 9, 20, 5, 3),        # C % 16 != 0: register kernels chained through res_post
    (1, 24, 32, 16, 9, 20, 5, 4),        # more inputs than one launch sums
    (1, 8, 8, 16, 3, 1, 1, 2),           # 3x3
]

WGRAD_MULTI_CASES = [
    (2, 24, 32, 16, 9, 20, 5, 3),        # one half-height tile pair per residue class (the ASPP shape in small)
    (1, 140, 270, 32, 9, 20, 5, 3),      # several tiles in both directions with real halos, ragged last tiles
    (1, 40, 70, 16, 9, 4, 1, 2),         # two branches, dil 1: four row tiles, two column tiles
    (2, 64, 128, 48, 9, 20, 5, 3),       # three channel groups
    (1, 67, 33, 16, 9, 20, 5, 3),        # 14 lattice rows: a 13-row and a 1-row tile (fewer rows than fetch slots)
    (1, 23, 37, 72, 9, 20, 5, 3),        # C % 16 != 0: one register-kernel launch per branch
    (1, 24, 32, 16, 9, 20, 5, 4),        # four branches: three fused + one single
    (1, 8, 8, 16, 3, 1, 1, 2),           # 3x3
]

FANOUT_CASES = [
    (2, 24, 32, 16, 9, 20, 5, 3), (1, 140, 270, 32, 9, 20, 5, 3), (1, 40, 70, 16, 9, 4, 1, 2), (2, 64, 128, 48, 9, 20, 5, 3),
    (1, 23, 37, 72, 9, 20, 5, 3), (1, 24, 32, 16, 9, 20, 5, 5), (1, 8, 8, 16, 3, 1, 1, 2),
]

LONE_WAVE_CASES = [
    # N, H, W, C: shapes that walk the lone-wave fan-out kernel's item pipeline (dwconv_lw.hip), 9x9 / dilation 5 / 3 branches
    (1, 128, 256, 32),       # the ASPP map: 50 items per (image, channel group), every item with 4 column tiles
    (2, 65, 130, 16),        # H, W multiples of dil; 13-row tiles exactly
    (1, 131, 523, 16),       # three row tiles (one of a single row), three column tiles per class, ragged ones
    (3, 7, 9, 16),           # a residue class of 2 x 2 pixels: one short item per class, single column tile
    (1, 5, 5, 48),           # one pixel per class, three channel groups
    (1, 266, 40, 16),        # five row tiles, 8 columns
    (2, 10, 30, 16, 1),      # dilation 1, ONE work item per workgroup (the item loop's exit on its first pass)
    (1, 20, 30, 32, 1),      # dilation 1, two items per workgroup (nothing to stage behind the second)
    (1, 40, 120, 16, 2),     # dilation 2: four classes of 20 x 60, two row tiles and two column tiles each
]

LATTICE_CASES = [
    # N, H, W, C, k, pad, dil, branches -- bf16 only (the lattice-planar intermediates of the replaced ASPP branches)
    (2, 24, 32, 16, 9, 20, 5, 3),        # H, W not multiples of dil: classes one row / column shorter, padded cells
    (1, 128, 256, 32, 9, 20, 5, 3),      # the ASPP map itself: 26 x 52 lattice, one tile per class (last row / column padded)
    (1, 140, 270, 32, 9, 20, 5, 3),      # several tiles per class with real halos, ragged last tiles
    (2, 40, 70, 16, 9, 4, 1, 2),         # two branches, dil 1: one class, many tiles, nothing padded
    (2, 64, 128, 48, 9, 20, 5, 2),       # three channel groups (three planes), two branches
    (3, 65, 130, 16, 9, 20, 5, 3),       # H, W multiples of dil: no padded cells; tail rows of the plane only
]


def lone_wave_case(case):
    """A LONE_WAVE_CASES row as (N, H, W, C, k, pad, dil, 3)."""
    d = case[4] if len(case) > 4 else 5
    return tuple(case[:4]) + (9, 4 * d, d, 3)


def mfma(dt, case):
    """The matrix-core kernels' domain (dwconv_mfma.hip, dwconv_lw.hip)."""
    return dt == "bf16" and case[4] == 9 and case[3] % 16 == 0


def chunks(n):
    """Branches per launch: 3 / 3 / ... / 2 or 1."""
    return [min(3, n - done) for done in range(0, n, 3)]


def fwd_kernel(dt, case):
    return "dw_mfma_fwd_kernel<1,false>" if mfma(dt, case) else f"dwconv_fwd_kernel<{dt}>"


def wgrad_kernel(dt, case):
    return "dw_mfma_wgrad_kernel" if mfma(dt, case) else f"dwconv_wgrad_kernel<{dt}>"


def sum_kernels(dt, case):
    """Every kernel kd_dwconv_fwd_sum notes for the row, in order: one launch for up to three matrix-core inputs, else the first term
    plain and the others through the register kernel's res_post epilogue."""
    n = case[7]
    if mfma(dt, case) and n <= 3:
        return [f"dw_mfma_fwd_kernel<{n},false>"]
    return [fwd_kernel(dt, case)] + [f"dwconv_fwd_kernel<{dt}>"] * (n - 1)


def fanout_kernels(dt, case):
    """... kd_dwconv_fwd_fanout: three bf16 9x9 branches on the lone-wave kernel, two on the 8-wave fan-out, one alone."""
    if not mfma(dt, case):
        return [f"dwconv_fwd_kernel<{dt}>"] * case[7]
    return ["dw_lw_fan3_kernel" if m == 3 else f"dw_mfma_fwd_kernel<{m},true>" if m == 2 else "dw_mfma_fwd_kernel<1,false>" for m in chunks(case[7])]


def wgrad_multi_kernels(dt, case):
    """... kd_dwconv_wgrad_multi: three or two branches fused, one alone."""
    if not mfma(dt, case):
        return [f"dwconv_wgrad_kernel<{dt}>"] * case[7]
    return [f"dw_mfma_wgrad_multi_kernel<{m}>" if m >= 2 else "dw_mfma_wgrad_kernel" for m in chunks(case[7])]


def lattice_kernels(case):
    """The fan-out, the sum and the multi weight gradient on lattice-planar intermediates (bf16)."""
    n = case[7]
    return f"dw_mfma_fwd_kernel<{n},true,lattice>", f"dw_mfma_fwd_kernel<{n},false,lattice>", f"dw_mfma_wgrad_multi_kernel<{n},lattice>"
