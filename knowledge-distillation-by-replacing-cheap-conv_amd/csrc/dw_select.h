// Which kernel the depthwise entry points (dwconv.hip: kd_dwconv_fwd, _fwd_sum, _fwd_fanout, _wgrad, _wgrad_multi and their
// lattice twins) run for a call, and on what grid: a pure function of the descriptor, a few facts about the call and the A/B
// switches.  The launchers (dwconv.hip, dwconv_mfma.hip, dwconv_lw.hip) switch over the result; the two workspace queries and
// kd_dwconv_lattice_ok evaluate the same function with the facts a shape alone gives, so a query cannot disagree with the launch.
// No HIP and no getenv here: a plain host C++ compiler accepts this file, and tests/test_dw_select_host.py holds it against the
// restatement of tests/_dw_dispatch_cases.py.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/kdcc.h"

// One value per name the launchers note in the kernel-selection log (dw_kernel_name), then DW_EACH.
enum DwKernel {
    DW_REG_FWD_BF16, DW_REG_FWD_F32, DW_REG_WGRAD_BF16, DW_REG_WGRAD_F32,                    // dwconv.hip
    DW_MFMA_FWD_1, DW_MFMA_SUM_2, DW_MFMA_SUM_3, DW_MFMA_FAN_2, DW_MFMA_FAN_3,               // dwconv_mfma.hip
    DW_MFMA_SUM_2_LP, DW_MFMA_SUM_3_LP, DW_MFMA_FAN_2_LP, DW_MFMA_FAN_3_LP,
    DW_MFMA_WGRAD, DW_MFMA_WGRAD_2, DW_MFMA_WGRAD_3, DW_MFMA_WGRAD_2_LP, DW_MFMA_WGRAD_3_LP,
    DW_LW_FAN3,                                                                              // dwconv_lw.hip
    DW_EACH,   // not a kernel: no launch takes the branches together, the entry point makes one kd_dwconv_fwd / kd_dwconv_wgrad call per branch
};
static inline const char *dw_kernel_name(int k)
{
    static const char *const names[] = {
        "dwconv_fwd_kernel<bf16>", "dwconv_fwd_kernel<f32>", "dwconv_wgrad_kernel<bf16>", "dwconv_wgrad_kernel<f32>",
        "dw_mfma_fwd_kernel<1,false>", "dw_mfma_fwd_kernel<2,false>", "dw_mfma_fwd_kernel<3,false>", "dw_mfma_fwd_kernel<2,true>", "dw_mfma_fwd_kernel<3,true>",
        "dw_mfma_fwd_kernel<2,false,lattice>", "dw_mfma_fwd_kernel<3,false,lattice>", "dw_mfma_fwd_kernel<2,true,lattice>", "dw_mfma_fwd_kernel<3,true,lattice>",
        "dw_mfma_wgrad_kernel", "dw_mfma_wgrad_multi_kernel<2>", "dw_mfma_wgrad_multi_kernel<3>", "dw_mfma_wgrad_multi_kernel<2,lattice>", "dw_mfma_wgrad_multi_kernel<3,lattice>",
        "dw_lw_fan3_kernel"};
    return k >= 0 && k < DW_EACH ? names[k] : nullptr;
}

// Every KDCC_DW_* switch the three files read (dw_switches() in dwconv.hip builds it once per process); the defaults are the shipped configuration.
struct DwSwitches {
    int mfma = 1;                   // KDCC_DW_MFMA: 0 = always the register kernels
    int lattice = 1;                // KDCC_DW_LATTICE: 0 = kd_dwconv_lattice_ok says no (NHWC intermediates)
    int lw = 1;                     // KDCC_DW_LW: 0 = the fan-out of three on the 8-wave kernel
    int lw_order = 1;               // KDCC_DW_LW_ORDER: 0 = the lone-wave item list with the classes innermost (round 6's first order: the halo rows are fetched from HBM twice)
    int tile_s = 2, tile_r = 8;     // KDCC_DW_TILE: thread tile of dwconv_fwd_kernel, 2x8 | 2x4 | 4x4 (2x8 measured fastest at the student's shapes)
    int dbg = 0, lw_dbg = 0;        // KDCC_DW_DBG, KDCC_DW_LW_DBG: timing ablations, tuning build only
};

// What the kernels' translation units are built for; each asserts these against its own constants.
constexpr int DW_CG = 16;                              // channels per workgroup of every matrix-core kernel
constexpr int DW_MAXB = 3;                             // branches one launch takes
constexpr int DW_TLX = 52, DW_TLY = 26, DW_TLY_HALF = 13;   // lattice tile of a work item; the multi weight gradient and the lone-wave fan-out use half-height tiles
constexpr uint32_t DW_BUF_OOB = 0x80000000u;           // buffer offsets are 32-bit per image: an image stays below this many bytes
constexpr int DW_REG_CB = 64;                          // channels per workgroup of the register kernels
constexpr int DW_FWD_LDS = 146176, DW_FWD_LDS_PER_BRANCH = 4608;   // dynamic LDS: dw_mfma_fwd_kernel (+ one tap table per further branch),
constexpr int DW_WGRAD_LDS = 127008, DW_WGRAD_MULTI_LDS = 131296, DW_LW_LDS = 161088;   // the two weight-gradient kernels, dw_lw_fan3_kernel

static_assert(DW_MFMA_FAN_2 == DW_MFMA_SUM_2 + 2 && DW_MFMA_SUM_2_LP == DW_MFMA_SUM_2 + 4 && DW_MFMA_FAN_3_LP == DW_MFMA_FAN_2 + 5 && DW_MFMA_WGRAD_3_LP == DW_MFMA_WGRAD_2 + 3,
              "dw_select computes the branch-count / fan-out / lattice variants from the order of DwKernel");

const DwSwitches &dw_switches();   // dwconv.hip: the process's switches
// kd_internal_dw_lw_fanout (dwconv_lw.hip) beside KD_OK / an error: the item table of the geometry could not be allocated or
// uploaded, nothing was launched
constexpr int KD_DW_LW_NO_TABLE = 1;

enum DwOp { DW_FWD, DW_SUM, DW_FANOUT, DW_WGRAD, DW_WGRAD_MULTI };

// What the choice depends on besides the descriptor
struct DwFacts {
    bool aligned16;     // every tensor pointer of the call is 16-B aligned
    int ld_dy;          // pixel stride of the output gradients (weight gradients; ignored where they are lattice-planar)
    bool epilogue;      // a bias or an epilogue operand is present (DW_FWD)
    bool capturing;     // the stream is being captured (the lone-wave kernel's item table is uploaded with a synchronous copy)
};
// ... when only the shape is known (the workspace bounds, kd_dwconv_lattice_ok): the friendliest call of that shape
static inline DwFacts dw_shape_facts(const kd_dw_desc *d) { return DwFacts{true, d->C, false, false}; }

struct DwSel {
    DwKernel kernel;
    int nb, fan, lp;            // branches of the launch; fan-out (else sum); lattice-planar branch tensors
    int nty, ntx;               // tiles of a residue class (register forward kernel: thread tiles)
    int nitems, nseg, ncg;      // work items per (image, channel group), segments they are split into, channel groups
                                // (register kernels: nitems = groups of 16 thread tiles / lattice-row strips, nseg = N * dil^2)
    long long blocks;           // workgroups
    int lds;                    // dynamic LDS bytes
    int slabs;                  // weight gradients: [k*k][C] fp32 partial-sum slabs the launch writes PER BRANCH
    int tile_s, tile_r;         // register forward kernel: thread tile
};

// Branches [done, done + dw_chunk) go into one launch: 3 / 3 / ... / 2 or 1.  The launch loops and the workspace bound walk this.
static inline int dw_chunk(int n, int done) { return n - done < DW_MAXB ? n - done : DW_MAXB; }

static inline long long dw_lattice_rows(int N, int H, int W, int dil)
{
    if (N < 1 || H < 1 || W < 1 || dil < 1) return 0;
    const long long Ly = (H + dil - 1) / dil, Lx = (W + dil - 1) / dil;
    return ((long long)N * dil * dil * Ly * Lx + 255) / 256 * 256;   // a multiple of the 1x1 convs' M tile
}

// The segments a list of `ni` work items per (image, channel group) is split into, one workgroup each: one workgroup per CU at a
// time (LDS), so aim at two rounds of workgroups over the 256 CUs, but keep >= `per` items per workgroup.
static inline void dw_segments(const kd_dw_desc *d, long long ni, int per, DwSel &c)
{
    const long long groups = (long long)d->N * (d->C / DW_CG);
    c.nitems = (ni > (1 << 24) || groups < 1) ? 0 : (int)ni;
    long long s = groups < 1 ? 1 : (512 + groups - 1) / groups;
    if (s > ni / per) s = ni / per;
    if (s < 1) s = 1;
    c.nseg = (int)s;
    c.ncg = d->C / DW_CG;
    c.blocks = (long long)d->N * c.ncg * c.nseg;
}

// Work items of tly x DW_TLX lattice outputs, every tile of every residue class; >= 3 per workgroup so that the prefetch has
// something to overlap with and the per-workgroup set-up is amortised.  (A second, independent workgroup per CU on half-height
// items was built and measured slower -- the Toeplitz rebuilds multiply: profiles/r05_dw_anatomy.md, commit dc356ad.)
static inline void dw_split(const kd_dw_desc *d, int tly, DwSel &c)
{
    const int LH = (d->H + d->dil - 1) / d->dil, LW = (d->W + d->dil - 1) / d->dil;
    c.nty = (LH + tly - 1) / tly;
    c.ntx = (LW + DW_TLX - 1) / DW_TLX;
    dw_segments(d, (long long)c.nty * c.ntx * d->dil * d->dil, 3, c);
}

// The lone-wave fan-out walks a table of its NON-EMPTY 13 x 52 items (dwconv_lw.hip, item_table): their count, 0 = no table
// (tile indices and the dilation are bytes of a descriptor); >= 8 per workgroup so that the operand build (once per workgroup)
// and the pipeline fill stay small.
static inline void dw_lw_split(const kd_dw_desc *d, DwSel &c)
{
    const int dl = d->dil, LH = (d->H + dl - 1) / dl, LW = (d->W + dl - 1) / dl;
    c.nty = (LH + DW_TLY_HALF - 1) / DW_TLY_HALF;
    c.ntx = (LW + DW_TLX - 1) / DW_TLX;
    long long rows = 0, cols = 0;
    if (c.nty <= 255 && c.ntx <= 255 && dl <= 255)
        for (int r = 0; r < dl; ++r) {   // class r has ceil((H - r) / dl) lattice rows (none if r >= H)
            rows += r < d->H ? ((d->H - r + dl - 1) / dl + DW_TLY_HALF - 1) / DW_TLY_HALF : 0;
            cols += r < d->W ? ((d->W - r + dl - 1) / dl + DW_TLX - 1) / DW_TLX : 0;
        }
    dw_segments(d, rows * cols, 8, c);
}

// Can the fan-out / summing / multi-gradient launches of n branches run on lattice-planar intermediates?  The matrix-core
// kernels' shape conditions, plus: no work item of the fan-out may be empty while its padded cells exist -- they are zeroed by the
// item that owns them -- and a plane's rows must stay inside 32-bit buffer offsets.
static inline bool dw_lattice_ok(const kd_dw_desc *d, int n, const DwSwitches &sw)
{
    if (n < 2 || n > DW_MAXB || d->dtype != KD_BF16 || d->k != 9 || d->C % DW_CG != 0 || d->ldx % 8 != 0) return false;
    if (!sw.mfma || !sw.lattice) return false;
    const int Ly = (d->H + d->dil - 1) / d->dil, Lx = (d->W + d->dil - 1) / d->dil;
    const long long rpi = (long long)(d->dil * d->dil * Ly * Lx), plane = dw_lattice_rows(d->N, d->H, d->W, d->dil) * DW_CG;
    if (rpi * DW_CG * 2 >= (long long)DW_BUF_OOB || plane * (d->C / DW_CG) > 0x7fffffffLL) return false;
    if ((long long)d->H * d->W * d->ldx * 2 >= (long long)DW_BUF_OOB) return false;
    const int ry_last = Ly - (Ly - 1) / DW_TLY * DW_TLY, rx_last = Lx - (Lx - 1) / DW_TLX * DW_TLX;   // padded extent of the last tile row / column
    const bool short_y = (d->H % d->dil) != 0, short_x = (d->W % d->dil) != 0;                         // some classes are one row / column shorter
    return !((short_y && ry_last < 2) || (short_x && rx_last < 2));
}

// op: the entry point; n: the branches of ONE chunk (dw_chunk; 1 for DW_FWD / DW_WGRAD); lattice: the branch tensors -- the
// fan-out's outputs, the sum's inputs, the output gradients -- are lattice-planar.
static inline DwSel dw_select(DwOp op, const kd_dw_desc *d, int n, bool lattice, const DwFacts &f, const DwSwitches &sw)
{
    DwSel c{};
    const bool bf16 = d->dtype == KD_BF16, wgrad = op == DW_WGRAD || op == DW_WGRAD_MULTI;
    c.nb = n; c.fan = op == DW_FANOUT && n > 1; c.lp = lattice;
    // the second tensor's pixel stride: the output(s), or the output gradient(s); lattice-planar ones have none (their cells are dense)
    const bool dense = lattice && op != DW_SUM;
    const int ld2 = dense ? d->C : wgrad ? f.ld_dy : d->ldy;
    // The matrix-core kernels: bf16 9x9, whole 16-channel groups, 16-B pixels and pointers, 32-bit offsets.  Calls with a bias or an
    // epilogue stay on the register kernel: their extra operands are read per pixel in 32-B (16-channel) pieces there, which the
    // memory system serves at about a third of the rate of the register kernel's 128-B-per-pixel rows (measured: 1.22 vs 0.99 ms
    // at 4096 channels, mask + residual, 2 images).
    const bool mc = sw.mfma && bf16 && d->k == 9 && d->C % DW_CG == 0 && d->ldx % 8 == 0 && ld2 % 8 == 0 && f.aligned16 && !f.epilogue &&
                    (long long)d->N * d->H * d->W <= 0x7fffffffLL && (!lattice || dw_lattice_ok(d, n, sw));
    const long long img = (long long)d->H * d->W * 2;                 // bytes of an image per unit of pixel stride
    const bool x_fits = img * d->ldx < (long long)DW_BUF_OOB, both_fit = img * (d->ldx > ld2 ? d->ldx : ld2) < (long long)DW_BUF_OOB;
    auto fits = [&](void) { return c.nitems > 0 && c.blocks <= 0x7fffffffLL; };
    if (!wgrad && mc && n >= 1 && n <= DW_MAXB && !(op == DW_FWD && n != 1)) {
        if (c.fan && n == 3 && !lattice && sw.lw && !f.capturing && both_fit) {
            dw_lw_split(d, c);
            if (fits()) { c.kernel = DW_LW_FAN3; c.lds = DW_LW_LDS; return c; }
        }
        dw_split(d, DW_TLY, c);
        if (x_fits && fits()) {
            c.kernel = n == 1 ? DW_MFMA_FWD_1 : (DwKernel)((c.fan ? DW_MFMA_FAN_2 : DW_MFMA_SUM_2) + (lattice ? 4 : 0) + (n - 2));
            c.lds = DW_FWD_LDS + (n - 1) * DW_FWD_LDS_PER_BRANCH;
            return c;
        }
    }
    // (kd_dwconv_wgrad_multi checks its arguments one branch at a time, in the calls of a chunk that is not fused: ld_dy < C ends there)
    if (wgrad && mc && both_fit && (op == DW_WGRAD ? n == 1 : n >= 2 && n <= DW_MAXB && ld2 >= d->C)) {
        dw_split(d, op == DW_WGRAD ? DW_TLY : DW_TLY_HALF, c);
        if (fits()) {
            c.kernel = op == DW_WGRAD ? DW_MFMA_WGRAD : (DwKernel)(DW_MFMA_WGRAD_2 + (lattice ? 2 : 0) + (n - 2));
            c.lds = op == DW_WGRAD ? DW_WGRAD_LDS : DW_WGRAD_MULTI_LDS;
            c.slabs = d->N * c.nseg;
            return c;
        }
    }
    // the register kernels: one launch per branch
    c = DwSel{};
    c.nb = 1;
    c.kernel = DW_EACH;
    const int LH = (d->H + d->dil - 1) / d->dil, LW = (d->W + d->dil - 1) / d->dil;
    c.ncg = (d->C + DW_REG_CB - 1) / DW_REG_CB;
    c.nseg = d->N * d->dil * d->dil;
    if (op == DW_FWD) {
        c.kernel = bf16 ? DW_REG_FWD_BF16 : DW_REG_FWD_F32;
        c.tile_s = sw.tile_s; c.tile_r = sw.tile_r;
        c.nty = (LH + c.tile_s - 1) / c.tile_s;
        c.ntx = (LW + c.tile_r - 1) / c.tile_r;
        c.nitems = (c.nty * c.ntx + 15) / 16;
        c.blocks = (long long)c.nitems * c.nseg * c.ncg;
    } else if (op == DW_WGRAD) {
        c.kernel = bf16 ? DW_REG_WGRAD_BF16 : DW_REG_WGRAD_F32;
        c.nitems = c.nseg * LH;             // strips: one lattice row of one class
        c.slabs = (c.nitems + 15) / 16;
        c.blocks = (long long)c.slabs * c.ncg * d->k;
    }
    return c;
}

// Workspace of kd_dwconv_wgrad: pointer alignment is not known when the caller asks, so the larger of the two plans it decides between.
static inline size_t dw_wgrad_workspace(const kd_dw_desc *d, const DwSwitches &sw)
{
    DwFacts unaligned = dw_shape_facts(d);
    unaligned.aligned16 = false;
    const int reg = dw_select(DW_WGRAD, d, 1, false, unaligned, sw).slabs, mc = dw_select(DW_WGRAD, d, 1, false, dw_shape_facts(d), sw).slabs;
    return (size_t)(reg > mc ? reg : mc) * d->k * d->k * d->C * sizeof(float);
}
// ... of kd_dwconv_wgrad_multi (and its lattice twin): the largest chunk's need -- a fused chunk's slabs for each of its branches,
// or one branch's workspace where the chunk runs one launch per branch
static inline size_t dw_wgrad_multi_workspace(const kd_dw_desc *d, int n, const DwSwitches &sw)
{
    size_t need = dw_wgrad_workspace(d, sw);
    for (int done = 0, m; done < n; done += m) {
        m = dw_chunk(n, done);
        const size_t fused = (size_t)dw_select(DW_WGRAD_MULTI, d, m, false, dw_shape_facts(d), sw).slabs * m * d->k * d->k * d->C * sizeof(float);
        if (fused > need) need = fused;
    }
    return need;
}
