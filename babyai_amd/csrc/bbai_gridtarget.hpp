// bbai_gridtarget.hpp -- the geometry of the 64-byte pieces that the registered full-grid target's delta render stores (k_grid_delta<TS>,
// bbai_griddelta.hpp; bbai_set_grid_target, include/bbai_grid_target.h), and that kernel's launch shape.  The target's record and its
// planner are bbai_target.hpp's, shared with the 7x7 view's target.
// Plain C++: no HIP, no device code (tests/test_grid_delta_host.py compiles it with g++).
#pragma once
#include <stdint.h>
#include "bbai_types.hpp"

namespace bbai {

constexpr int GRID_PIECE = 64;            // the store unit, as the view's delta renders' (bbai_render.hpp PIECE_BYTES, bbai_viewpx.hpp VIEW_PIECE)

// ---- the pieces of a frame ---------------------------------------------------------------------------------------------------------
// A frame is H ts pixel rows of RB = 3 W ts bytes; F = 3 W H ts^2 bytes.  RB is no multiple of 64 for most W (96 B at W = 4 / ts 8,
// 168 B at W = 7, 528 B at W = 22), so piece p = bytes [64 p, 64 p + 64) may span two pixel rows -- never three: RB >= 64 from W = 3 on,
// grid_geom_ok.  A TILE row is ts pixel rows = 3 W ts^2 bytes, a multiple of 64 at tile sizes 8 / 16 / 32 (192 W, 768 W, 3072 W): at
// these sizes both pixel rows of a piece lie in one tile row and every piece has ONE segment.  grid_piece_segments does not rely on
// that (it answers for any row length); the row walk below it does, and says so.  Divides by RB and by 3 are multiply-high (exact for
// every byte offset of the largest frame, 25 x 25 at 32: the host test walks every piece of every level's grid).
struct GridGeom {
    int W, H, ts, lg;             // lg = log2(ts)
    uint32_t RB;                  // bytes of a pixel row
    uint32_t NP;                  // pieces of a frame
    uint64_t rb_magic;            // 2^40 / RB + 1
};
constexpr uint64_t GRID_MAGIC3 = ((1ull << 40) / 3) + 1;

BB_HD bool grid_geom_ok(int W, int H, int ts) { return (ts == 8 || ts == 16 || ts == 32) && W >= 3 && W <= 25 && H >= 1 && H <= 25; }
BB_HD GridGeom grid_geom(int W, int H, int ts) {
    GridGeom g;
    g.W = W; g.H = H; g.ts = ts; g.lg = ts == 8 ? 3 : ts == 16 ? 4 : 5;
    g.RB = (uint32_t)(3 * W * ts);
    g.NP = (uint32_t)(3 * W * H * ts * ts / GRID_PIECE);
    g.rb_magic = (1ull << 40) / g.RB + 1;
    return g;
}
BB_HD uint32_t grid_div_rb(const GridGeom& g, uint32_t b) { return (uint32_t)(((uint64_t)b * g.rb_magic) >> 40); }       // b / RB, b < 2^21
BB_HD uint32_t grid_col(const GridGeom& g, uint32_t o) { return (uint32_t)((((uint64_t)(o >> g.lg)) * GRID_MAGIC3) >> 40); }   // o / (3 ts), o < RB

// Columns x0 .. x1 as a mask
BB_HD uint32_t grid_cols(uint32_t x0, uint32_t x1) { return (2u << x1) - (1u << x0); }

// Piece p's segments, at most two: (tile row y, mask of the columns x whose cells it holds bytes of).  Two pixel rows of one tile row
// are one segment.
struct GridSeg { int y; uint32_t cols; };
struct GridSegs { int n; GridSeg s[2]; };
BB_HD GridSegs grid_piece_segments(const GridGeom& g, uint32_t p) {
    GridSegs r;
    const uint32_t b0 = p * GRID_PIECE;
    const uint32_t r0 = grid_div_rb(g, b0), o0 = b0 - r0 * g.RB;
    const uint32_t e0 = o0 + GRID_PIECE < g.RB ? o0 + GRID_PIECE : g.RB;                 // the piece's bytes of pixel row r0: [o0, e0)
    r.n = 1;
    r.s[0].y = (int)(r0 >> g.lg);
    r.s[0].cols = grid_cols(grid_col(g, o0), grid_col(g, e0 - 1));
    r.s[1].y = 0; r.s[1].cols = 0;
    if (o0 + GRID_PIECE > g.RB) {                                                         // ... and [0, e1) of pixel row r0 + 1
        const uint32_t e1 = o0 + GRID_PIECE - g.RB;
        const int y1 = (int)((r0 + 1) >> g.lg);
        const uint32_t c1 = grid_cols(0, grid_col(g, e1 - 1));
        if (y1 == r.s[0].y) r.s[0].cols |= c1;
        else { r.n = 2; r.s[1].y = y1; r.s[1].cols = c1; }
    }
    return r;
}
BB_HD GridSegs grid_piece_segments(int W, int ts, uint32_t p) { return grid_piece_segments(grid_geom(W, 1, ts), p); }      // (a piece's segments do not depend on H)

// Is piece p dirty -- does one of its segments meet a changed cell?  rows[y] bit x = cell (x, y) changed.
BB_HD bool grid_piece_dirty(const GridGeom& g, uint32_t p, const uint32_t* rows) {
    const GridSegs s = grid_piece_segments(g, p);
    return (rows[s.s[0].y] & s.s[0].cols) != 0 || (s.n > 1 && (rows[s.s[1].y] & s.s[1].cols) != 0);
}

// Every piece is judged once, in its tile row: row y's pieces are [grid_row_first(y), grid_row_first(y + 1)) (grid_row_first(H) = NP) --
// a tile row being a whole number of pieces at tile sizes 8 / 16 / 32, a row is looked at iff it has a changed cell itself.
BB_HD uint32_t grid_row_first(const GridGeom& g, int y) { return (uint32_t)y * ((g.RB << g.lg) / GRID_PIECE); }
static_assert((3 * 8 * 8) % GRID_PIECE == 0, "a tile row, 3 W ts^2 bytes, is a whole number of pieces from tile size 8 on");

// ---- k_grid_delta's launch shape (bbai_griddelta.hpp) ------------------------------------------------------------------------------
// A block works on a GROUP of envs at a time; its LDS planes hold the group's record rows (dwords) and tile ids (bytes), every lane
// carrying GRIDDELTA_ROW_UNROLL dwords and GRIDDELTA_ID_UNROLL ids of the next group in registers.
constexpr int GRIDDELTA_BLOCK = 512;
constexpr int GRIDDELTA_MAX_ENVS = 32;           // envs per group at most (the per-env LDS arrays; a listed row is env * 32 + y)
constexpr int GRIDDELTA_ROW_UNROLL = 4;          // record-row dwords per lane and group
constexpr int GRIDDELTA_ID_UNROLL = 8;           // cells per lane and group
constexpr int GRIDDELTA_APP = GRIDDELTA_ROW_UNROLL * GRIDDELTA_BLOCK;      // dwords of record rows a group may have
constexpr int GRIDDELTA_IDS = GRIDDELTA_ID_UNROLL * GRIDDELTA_BLOCK;       // cells a group may have
constexpr int GRIDDELTA_BPC = 2;                 // persistent blocks per CU

// Envs per group at most for a W x H grid with record rows of ES bytes (a multiple of 4): what the planes hold.
inline int griddelta_group(int W, int H, int ES) {
    int g = GRIDDELTA_MAX_ENVS;
    if (GRIDDELTA_IDS / (W * H) < g) g = GRIDDELTA_IDS / (W * H);
    if (GRIDDELTA_APP / (H * ES / 4) < g) g = GRIDDELTA_APP / (H * ES / 4);
    return g < 1 ? 1 : g;
}
// The launch: envs per group and groups for a batch of n envs on `blocks` persistent blocks.  asked > 0 (option "grid_delta_group"):
// that many envs per group, clamped to what the planes hold; else as many as they hold, fewer while that still leaves a group per block.
struct GridDeltaShape { int envs_per_group; int64_t groups; };
inline GridDeltaShape griddelta_shape(int64_t n, int64_t blocks, int W, int H, int ES, int asked) {
    const int cap = griddelta_group(W, H, ES);
    int64_t g = asked > 0 ? asked : n / (blocks > 0 ? blocks : 1);
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return GridDeltaShape{(int)g, (n + g - 1) / g};
}

}  // namespace bbai
