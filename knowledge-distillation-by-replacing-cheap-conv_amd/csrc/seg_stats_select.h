// Which kernel kd_seg_class_stats (seg_stats_ops.hip) runs for a call, and on what grid: a pure function of the shapes, the tile size
// and the pointer value.  The launcher checks its arguments, calls the selector, notes seg_stats_kernel_name(sel.kernel) and launches
// what sel says.  No HIP, no getenv and no globals here: a plain host C++ compiler accepts this file, and
// tests/test_cityscapes_uniform_host.py holds it to both sides of every gate.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "seg_data_select.h"

enum SegStatsKernel { SSK_STATS_1, SSK_STATS_16, SEG_STATS_COUNT };
static inline const char *seg_stats_kernel_name(int k)
{
    static const char *const names[] = {"seg_class_stats_kernel<1>", "seg_class_stats_kernel<16>"};
    static_assert(sizeof(names) / sizeof(names[0]) == SEG_STATS_COUNT, "one name per kernel value");
    return k >= 0 && k < SEG_STATS_COUNT ? names[k] : nullptr;
}

// What seg_stats_ops.hip is built for; it aliases these or static_asserts against them.
constexpr int SEG_STATS_TPB = 256;              // threads of every workgroup
constexpr int SEG_STATS_MAX_CLASSES = 64;       // the per-wave partials in LDS are sized for this many
constexpr long long SEG_STATS_WG_BYTES = 1 << 16;   // labels one workgroup sums before it flushes: rows of one tile
constexpr unsigned SEG_STATS_MAX_GRID = 1u << 20;   // workgroups launched at most; each walks its units with the grid as stride

struct SegStatsSel {
    SegStatsKernel kernel;
    int launch;             // 0: H < tile or W < tile, there is no tile and nothing to launch
    int vec;                // labels a thread loads at once: 1 or 16
    int th, tw;             // tiles down and across: H / tile, W / tile (remainder rows and columns belong to no tile)
    int rows;               // rows of a tile one unit covers
    int chunks;             // units a tile is cut into: ceil(tile / rows)
    long long units;        // n * th * tw * chunks
    unsigned grid;          // min(units, SEG_STATS_MAX_GRID)
};

static inline bool seg_stats_classes_ok(int32_t c) { return c >= 1 && c <= SEG_STATS_MAX_CLASSES; }

// Rows of one tile a workgroup may sum into its 32-bit partials when it aims at `budget` bytes of labels.
// The bound: a unit of R rows of a tile holds at most R * tile labels of one class; their column sum is at most
// R * (0 + 1 + ... + tile - 1) = R * tile * (tile - 1) / 2, and their row sum, taken relative to the unit's first row, at most
// tile * R * (R - 1) / 2, which is no larger while R <= tile.  So the uint32 partials are exact while R <= tile and
// R * tile * (tile - 1) / 2 < 2^32; the 64-bit totals in `stats` hold any tile up to SEG_MAX_SIDE (below 2^45).
static inline int seg_stats_rows(int32_t tile, long long budget)
{
    const long long t = tile, row_sum = t * (t - 1) / 2;
    long long rows = budget / t;
    if (row_sum > 0 && rows > 0xffffffffLL / row_sum) rows = 0xffffffffLL / row_sum;     // SEG_MAX_SIDE: 8 rows still fit
    if (rows > t) rows = t;
    return rows < 1 ? 1 : (int)rows;
}

// kd_seg_class_stats.  16-B loads of 16 labels when the labels are 16-B aligned and both W and the tile are multiples of 16: every
// row of every tile then starts at a multiple of 16 bytes and is whole 16-B pieces.  Byte loads otherwise.
static inline SegStatsSel seg_stats_select(const void *targets, int64_t n, int32_t H, int32_t W, int32_t tile)
{
    SegStatsSel s{};
    const bool vec = seg_aligned16(targets) && W % 16 == 0 && tile % 16 == 0;
    s.kernel = vec ? SSK_STATS_16 : SSK_STATS_1;
    s.vec = vec ? 16 : 1;
    s.th = H / tile, s.tw = W / tile;
    s.rows = seg_stats_rows(tile, SEG_STATS_WG_BYTES);
    s.chunks = (tile + s.rows - 1) / s.rows;
    s.units = (long long)n * s.th * s.tw * s.chunks;
    s.launch = s.units > 0;
    s.grid = (unsigned)(s.units < (long long)SEG_STATS_MAX_GRID ? s.units : (long long)SEG_STATS_MAX_GRID);
    return s;
}
