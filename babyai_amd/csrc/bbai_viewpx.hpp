// bbai_viewpx.hpp -- the agent's 7x7 view as pixels at tile sizes 16 and 32: k_view_pixels<TS>, RGBImgPartialObsWrapper(env, tile_size)
// .observation of rows of an ENCODED observation buffer (bbai_render_view), and the delta render of a whole batch into the registered
// target of that size (k_view_delta<TS>, with k_view_ids behind a whole-frame render that has to fill the shadow).  Tile size 8 is
// bbai_render.hpp's (k_render and its kin, with its own delta render); k_view_pixels is a stand-alone full render in the shape of
// k_render_grid, with GridTile<TS>'s piece arithmetic.
//
// The first part is plain C++ -- which cells a 64-byte piece of a frame is drawn from, which the host tests compile with g++
// (tests/test_view_delta_host.py).  The kernels below it are part of bbai_engine.hip's translation unit: included next to bbai_gridk.hpp,
// at global scope.  The launches are bbai_engine.hip's (render_view_launch, view_delta_launch).
#pragma once
#include "bbai_types.hpp"

namespace bbai {

// A frame at tile size TS in memory: 7 TS pixel rows of 21 TS bytes; the delta render's store unit is the 64-byte piece (DESIGN section 5a,
// "Store unit": whole 64-byte pieces run at 0.96 of whole-line time, 32- and 16-byte ones at 1.8-2.3 x).  147 TS^2 is a multiple of 128 at
// 16 and 32, so a piece never crosses a frame, and a tile row of the view -- TS pixel rows, 21 TS^2 bytes -- is PR whole pieces.
constexpr int VIEW_PIECE = 64;
template <int TS> struct ViewFrame {
    static_assert(TS == 16 || TS == 32, "tile size 8 is bbai_render.hpp's");
    static constexpr int ROW_BYTES = VIEW * TS * 3;                  // 336 / 672
    static constexpr int BYTES = ROW_BYTES * VIEW * TS;              // 37 632 / 150 528
    static constexpr int NP = BYTES / VIEW_PIECE;                    // pieces per frame: 588 / 2352
    static constexpr int PR = NP / VIEW;                             // pieces per tile row of the view: 84 / 336
    static_assert(BYTES % (2 * VIEW_PIECE) == 0 && NP % VIEW == 0, "whole pieces per frame and per tile row");
};
constexpr uint64_t VIEW_ROW0 = 0x40810204081ull;                     // the cells (x, 0): bits 7 x

// The cells (bit 7 x + y, as tile_id's `cell`) that piece p of a frame is drawn from: its four 16-byte chunks, each from its byte offset --
// pixel row b / ROW_BYTES, tile column (b % ROW_BYTES) / 3 TS.  A chunk never crosses a tile row (3 TS is a multiple of 16), a piece may
// (two cells), and at 16 it may span two pixel rows (336 is no multiple of 64).
template <int TS>
BB_HD constexpr uint64_t view_piece_cells(int p) {
    using F = ViewFrame<TS>;
    uint64_t m = 0;
    for (int c = 0; c < VIEW_PIECE / 16; ++c) {
        const int b = p * VIEW_PIECE + 16 * c;
        const int row = b / F::ROW_BYTES, xb = b - row * F::ROW_BYTES;
        m |= 1ull << (xb / (TS * 3) * VIEW + row / TS);
    }
    return m;
}

// What k_view_delta's piece table rests on: piece p of tile row r = p / PR touches the cells of piece p % PR of tile row 0, moved down r rows.
template <int TS>
BB_HD constexpr bool view_tile_rows_repeat() {
    using F = ViewFrame<TS>;
    for (int p = 0; p < F::NP; ++p) {
        const int r = p / F::PR, q = p - r * F::PR;
        if ((view_piece_cells<TS>(q) & ~VIEW_ROW0) != 0 || view_piece_cells<TS>(p) != view_piece_cells<TS>(q) << r) return false;
    }
    return true;
}
static_assert(view_tile_rows_repeat<16>() && view_tile_rows_repeat<32>(), "the pieces of every tile row touch the same columns");

}  // namespace bbai

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "bbai_kernels.hpp"
#include "bbai_gridk.hpp"

using namespace bbai;

// ------------------------------------------------------------------------------------------
// k_view_pixels : the 7x7 view of listed rows of an encoded buffer as uint8[7 TS][7 TS][3] frames (bbai_render_view)
// ------------------------------------------------------------------------------------------
// A frame is 7 x 7 atlas tiles, pixel row = view y, pixel column = view x (the encoding is indexed [x][y]: cell = 7 x + y), a flat run
// of 16-byte chunks: 147 TS^2 / 16 = 2352 / 9408 of them, 21 / 42 per pixel row, 3 / 6 per tile row (GridTile<TS>::PPT) -- so a chunk
// never crosses a tile row and is one 16-byte piece of one atlas tile.  Every divisor is a compile-time constant.
// A work item is envs_per_item frames (tile size 16: 4 = 150.5 KB) or one of `slices` parts of one frame (32: a frame is 150.5 KB; two
// halves when there are fewer frames than blocks).  Persistent blocks; per item
//   1. the item's encodings -- 3 bytes per cell, lane = cell, 147 contiguous bytes per env -- are ALREADY in registers (view_fetch): they
//      were loaded while the previous item's stores were issued, so no block ever waits for a load with no stores of its own in flight;
//   2. lane = cell turns them into tile ids in LDS (tile_id's rule, restated: lut[(cell == AGENT_CELL ? 256 : 0) + key]); ONE barrier
//      (the id planes are double-buffered: the next item's are written while slower waves still read this item's);
//   3. the next item's encodings are requested;
//   4. the frames leave as 16-byte nontemporal stores, VIEWPX_UNROLL chunks per lane in flight, a wave's 64 chunks contiguous (1 KiB).
// The atlas is in LDS at 16 (50 KB: two blocks per CU), read from global memory / L2 at 32 (181 KB), as k_render_grid<32> does.
// Writes nothing but `out`.  A row id outside [0, rows) draws every cell with the zero tile the atlas carries behind its last one.
// key = (o0 | o1 << 3 | o2 << 6) & 255: bytes no encoding holds (o0 > 7 ...) still index inside the lut.
constexpr int VIEWPX_BLOCK = 1024;
constexpr int VIEWPX_MAX_ENVS = 4;               // envs per work item
constexpr int VIEWPX_MAX_TILES = 64;             // atlas tiles (+ the zero tile)
constexpr int VIEWPX_UNROLL = 4;                 // 16-byte chunks per lane in flight
constexpr int VIEWPX_LUT_BYTES = 512;            // [2][256]
constexpr uint32_t VIEWPX_NONE = 0xffffffffu;    // view_fetch: no such row
static_assert(VIEWPX_MAX_ENVS * CELLS <= VIEWPX_BLOCK, "lane = cell of the item");

struct ViewPxArgs {
    const uint8_t* image;        // [rows][147], indexed [x][y][3]
    int64_t rows;
    const int64_t* ids;          // NULL: rows 0 .. count - 1
    int64_t count;
    uint8_t* out;
    const uint8_t* atlas;        // [n_tiles + 1][TS][TS][3], the last one all zero
    const uint8_t* lut;          // [2][256]
    int n_tiles;
    int envs_per_item, slices;   // one of them is 1
    int64_t items;
};

// Lane tid's cell of work item `item` (env tid / 49 of the item, cell tid % 49) as o0 | o1 << 8 | o2 << 16, VIEWPX_NONE where the item,
// the env or the row does not exist.
__device__ __forceinline__ uint32_t view_fetch(const ViewPxArgs& a, int64_t item, int tid) {
    if (item >= a.items) return VIEWPX_NONE;
    const int64_t first = a.slices > 1 ? item / a.slices : item * a.envs_per_item;
    const int e = tid / CELLS, cell = tid - e * CELLS;
    if (e >= a.envs_per_item || first + e >= a.count) return VIEWPX_NONE;
    const int64_t row = a.ids ? a.ids[first + e] : first + e;
    if (row < 0 || row >= a.rows) return VIEWPX_NONE;
    const uint8_t* p = a.image + row * OBS_BYTES + cell * 3;
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
}

// chunk j of a frame -> its 16 bytes of the atlas
template <int TS>
__device__ __forceinline__ const uint8_t* view_piece(const uint8_t* atlas, const uint8_t* ids, uint32_t j) {
    using G = GridTile<TS>;
    constexpr uint32_t PPR = VIEW * G::PPT;               // pieces per pixel row
    const uint32_t py = j / PPR, px = j - py * PPR;
    const uint32_t tx = px / G::PPT, part = px - tx * G::PPT;
    const uint32_t id = ids[tx * VIEW + py / TS];
    return atlas + id * G::BYTES + (py % TS) * (TS * 3) + part * G::P;
}

template <int TS>
__global__ __launch_bounds__(VIEWPX_BLOCK, 8) void k_view_pixels(ViewPxArgs a) {      // (8 waves per SIMD: two blocks per CU)
    using G = GridTile<TS>;
    static_assert(TS == 16 || TS == 32, "tile size 8 is k_render's");
    constexpr uint32_t F16 = CELLS * G::BYTES / 16;       // 16-byte chunks per frame
    __shared__ __attribute__((aligned(16))) uint8_t s_atlas[G::LDS ? (VIEWPX_MAX_TILES + 1) * G::BYTES : 16];
    __shared__ __attribute__((aligned(16))) uint8_t s_lut[VIEWPX_LUT_BYTES];
    __shared__ uint8_t s_ids[2][VIEWPX_MAX_ENVS * CELLS];
    const int tid = threadIdx.x;
    const uint8_t* atlas = a.atlas;
    if (G::LDS) {
        for (int k = tid; k < (a.n_tiles + 1) * G::BYTES / 16; k += VIEWPX_BLOCK) ((u32x4*)s_atlas)[k] = ((const u32x4*)a.atlas)[k];
        atlas = s_atlas;
    }
    if (tid < VIEWPX_LUT_BYTES / 16) ((u32x4*)s_lut)[tid] = ((const u32x4*)a.lut)[tid];
    uint32_t o = view_fetch(a, blockIdx.x, tid);
    __syncthreads();                                      // atlas and lut loaded
    u32x4* const out = (u32x4*)a.out;
    int b = 0;
    for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x, b ^= 1) {
        const int64_t first = a.slices > 1 ? item / a.slices : item * a.envs_per_item;      // first output frame of the item
        const uint32_t slice = (uint32_t)(item - first * a.slices);                         // (0 unless sliced)
        const uint32_t ne = a.slices > 1 ? 1u : (uint32_t)(a.count - first < a.envs_per_item ? a.count - first : a.envs_per_item);
        if (tid < VIEWPX_MAX_ENVS * CELLS) {
            const int cell = tid % CELLS;
            const uint32_t key = ((o & 255u) | ((o >> 8) & 255u) << 3 | ((o >> 16) & 255u) << 6) & 255u;
            s_ids[b][tid] = o == VIEWPX_NONE ? (uint8_t)a.n_tiles : s_lut[(cell == AGENT_CELL ? 256 : 0) + key];
        }
        __syncthreads();                                  // (the one barrier of an item: the other id plane is the next item's)
        o = view_fetch(a, item + gridDim.x, tid);         // the next item's encodings, under this item's stores
        // chunks [q0, q1) of the item, counted from its first frame's first chunk
        const uint32_t q0 = a.slices > 1 ? slice * F16 / (uint32_t)a.slices : 0u;
        const uint32_t q1 = a.slices > 1 ? (slice + 1) * F16 / (uint32_t)a.slices : ne * F16;
        u32x4* const base = out + first * (int64_t)F16;
        const uint8_t* const ids = s_ids[b];
        for (uint32_t qb = q0 + tid; qb < q1; qb += VIEWPX_UNROLL * VIEWPX_BLOCK) {
            u32x4 v[VIEWPX_UNROLL];
#pragma unroll
            for (int u = 0; u < VIEWPX_UNROLL; ++u) {
                const uint32_t q = qb + u * VIEWPX_BLOCK < q1 ? qb + u * VIEWPX_BLOCK : q1 - 1;     // (past the end: a chunk of the item, not stored)
                const uint32_t e = q / F16, j = q - e * F16;
                v[u] = *(const u32x4*)view_piece<TS>(atlas, ids + e * CELLS, j);
            }
#pragma unroll
            for (int u = 0; u < VIEWPX_UNROLL; ++u)
                if (qb + u * VIEWPX_BLOCK < q1) __builtin_nontemporal_store(v[u], base + qb + u * VIEWPX_BLOCK);
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_view_delta : a whole batch into the registered target of this tile size, storing only what changed (bbai_render_view)
// ------------------------------------------------------------------------------------------
// The registered buffer holds the previous frame of every env and the handle's shadow plane the atlas tile id of every cell of it
// (uint8[n][49], as at tile size 8: bbai_render.hpp, k_render_delta).  A cell whose id is unchanged has unchanged bytes, so only the 64-byte
// pieces that are drawn from a changed cell are stored (view_piece_cells above).  Persistent blocks over groups of G envs, assigned
// statically (no ticket counter: one counter's rate would be the bound); per group
//   A  one wave per env, lane = cell: the new tile id (tile_id's rule as k_view_pixels restates it), the old one from the shadow, a ballot
//      gives the env's 49-bit dirty mask, the changed ids go back to the shadow; the same wave lists the env's dirty pieces -- only the tile
//      rows that hold a dirty cell are looked at, a lane per piece tests (dirty columns of the row & the piece's columns: s_pm, PR entries),
//      a ballot compacts them into the WAVE's own list (no LDS atomic);
//   barrier; the next group's encodings and shadow bytes are requested;
//   B  the whole block stores the group's listed pieces, 16 bytes per lane through view_piece<TS>, VIEWDELTA_UNROLL chunks per lane in
//      flight: the W lists are walked as one run (their running counts in s_cum), so the stores are balanced over the group -- an env
//      that was reset (49 dirty cells) is shared by every wave, a group where nothing changed (most env-steps) costs two barriers;
//   barrier (the lists and ids are read before the next group writes them).
// The atlas is in LDS at 16, read from global memory / L2 at 32, as in k_view_pixels.  Writes the shadow and `out`, nothing else.
constexpr int VIEWDELTA_BLOCK = 512;
constexpr int VIEWDELTA_WAVES = VIEWDELTA_BLOCK / 64;
constexpr int VIEWDELTA_UNROLL = 4;              // 16-byte chunks per lane in flight
template <int TS> struct ViewDelta {
    static constexpr int EPW = TS == 16 ? 2 : 1;                     // envs per wave and group
    static constexpr int G = VIEWDELTA_WAVES * EPW;                  // envs per group: 16 / 8 (602 KB / 1.2 MB of frames)
    static constexpr int CAP = EPW * ViewFrame<TS>::NP;              // entries of a wave's list: every piece of its envs
    static_assert(G * ViewFrame<TS>::NP <= 65536, "a list entry (env of the group, piece) fits 16 bits");
};

struct ViewDeltaArgs {
    const uint8_t* image;        // [n][147], indexed [x][y][3]
    int64_t n;
    uint8_t* out;                // [n][7 TS][7 TS][3], 64-byte aligned
    uint8_t* shadow;             // [n][49]
    const uint8_t* atlas;        // [n_tiles + 1][TS][TS][3]
    const uint8_t* lut;          // [2][256]
    int n_tiles;
};

template <int TS>
__global__ __launch_bounds__(VIEWDELTA_BLOCK, 4) void k_view_delta(ViewDeltaArgs a) {      // (4 waves per SIMD: two blocks per CU)
    using GT = GridTile<TS>;
    using F = ViewFrame<TS>;
    using D = ViewDelta<TS>;
    constexpr int W = VIEWDELTA_WAVES, T = VIEWDELTA_BLOCK, EPW = D::EPW, G = D::G;
    constexpr uint32_t F16 = F::BYTES / 16;               // 16-byte chunks per frame
    __shared__ __attribute__((aligned(16))) uint8_t s_atlas[GT::LDS ? (VIEWPX_MAX_TILES + 1) * GT::BYTES : 16];
    __shared__ __attribute__((aligned(16))) uint8_t s_lut[VIEWPX_LUT_BYTES];
    __shared__ uint64_t s_pm[F::PR];                      // the columns (bits 7 x) piece q of a tile row is drawn from
    __shared__ uint8_t s_ids[G * CELLS];
    __shared__ uint16_t s_wl[W][D::CAP];                  // per wave: (env of the group) * NP + piece
    __shared__ uint32_t s_cum[W];                         // entries of lists 0 .. w
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* atlas = a.atlas;
    if (GT::LDS) {
        for (int k = tid; k < (a.n_tiles + 1) * GT::BYTES / 16; k += T) ((u32x4*)s_atlas)[k] = ((const u32x4*)a.atlas)[k];
        atlas = s_atlas;
    }
    if (tid < VIEWPX_LUT_BYTES / 16) ((u32x4*)s_lut)[tid] = ((const u32x4*)a.lut)[tid];
    for (int q = tid; q < F::PR; q += T) s_pm[q] = view_piece_cells<TS>(q);
    const int64_t ngroups = (a.n + G - 1) / G;
    // phase A's inputs of group `grp`, loaded ahead: the 3 encoding bytes (o0 | o1 << 8 | o2 << 16) and the old id of this lane's cell in each of the wave's envs
    uint32_t o[EPW], old[EPW];
    auto load = [&](int64_t grp) {
#pragma unroll
        for (int j = 0; j < EPW; ++j) {
            const int64_t env = grp * G + wave + j * W;
            o[j] = old[j] = 0;
            if (grp < ngroups && lane < CELLS && env < a.n) {
                const uint8_t* p = a.image + env * OBS_BYTES + lane * 3;
                o[j] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
                old[j] = a.shadow[env * CELLS + lane];
            }
        }
    };
    int64_t g = blockIdx.x;
    load(g);
    __syncthreads();                                      // atlas, lut and piece table loaded
    for (; g < ngroups; g += gridDim.x) {
        const int64_t env0 = g * G;
        const int ne = (int)(a.n - env0 < G ? a.n - env0 : G);
        // A: new ids, dirty masks, shadow write-back, the wave's list of dirty pieces
        uint32_t cnt = 0;
        uint16_t* const wl = s_wl[wave];
#pragma unroll
        for (int j = 0; j < EPW; ++j) {
            const int e = wave + j * W;
            const bool live = lane < CELLS && e < ne;
            const uint32_t key = ((o[j] & 255u) | ((o[j] >> 8) & 255u) << 3 | ((o[j] >> 16) & 255u) << 6) & 255u;
            const uint32_t id = live ? s_lut[(lane == AGENT_CELL ? 256 : 0) + key] : 0;
            const bool d = live && id != old[j];
            const uint64_t m = __ballot(d);
            if (live) s_ids[e * CELLS + lane] = (uint8_t)id;
            if (d) a.shadow[(env0 + e) * CELLS + lane] = (uint8_t)id;
            if (!m) continue;
            for (int r = 0; r < VIEW; ++r) {
                const uint64_t cols = (m >> r) & VIEW_ROW0;          // the dirty cells (x, r), as bits 7 x
                if (!cols) continue;
                for (int q0 = 0; q0 < F::PR; q0 += 64) {
                    const int q = q0 + lane;
                    const bool dp = q < F::PR && (cols & s_pm[q]) != 0;
                    const uint64_t b = __ballot(dp);
                    if (dp) wl[cnt + __builtin_popcountll(b & ((1ull << lane) - 1))] = (uint16_t)(e * F::NP + r * F::PR + q);
                    cnt += (uint32_t)__builtin_popcountll(b);
                }
            }
        }
        if (lane == 0) s_cum[wave] = cnt;
        __syncthreads();                                  // ids, lists and counts written
        load(g + gridDim.x);                              // the next group's inputs ride under this group's stores
        // B: the W lists as one run of pieces, 4 chunks each
        uint32_t cum[W];
        uint32_t run = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) { run += s_cum[w]; cum[w] = run; }
        const uint32_t nq = run * (VIEW_PIECE / 16);
        u32x4* const base = (u32x4*)a.out + env0 * (int64_t)F16;
        for (uint32_t ib = tid; ib < nq; ib += VIEWDELTA_UNROLL * T) {
            u32x4 v[VIEWDELTA_UNROLL];
            uint32_t dst[VIEWDELTA_UNROLL];
#pragma unroll
            for (int u = 0; u < VIEWDELTA_UNROLL; ++u) {
                const uint32_t i = ib + u * T < nq ? ib + u * T : nq - 1;      // (past the end: a chunk of the group, not stored)
                const uint32_t k = i / (VIEW_PIECE / 16);
                uint32_t w = 0, first = 0;                // the list that holds entry k of the run, and the entries in front of it
#pragma unroll
                for (int x = 0; x < W - 1; ++x)
                    if (k >= cum[x]) { w = x + 1; first = cum[x]; }
                const uint32_t entry = s_wl[w][k - first];
                const uint32_t e = entry / F::NP, j = (entry - e * F::NP) * (VIEW_PIECE / 16) + (i & (VIEW_PIECE / 16 - 1));
                v[u] = *(const u32x4*)view_piece<TS>(atlas, s_ids + e * CELLS, j);
                dst[u] = e * F16 + j;
            }
#pragma unroll
            for (int u = 0; u < VIEWDELTA_UNROLL; ++u)
                if (ib + u * T < nq) __builtin_nontemporal_store(v[u], base + dst[u]);
        }
        __syncthreads();                                  // the lists and ids are read: the next group may write them
    }
}

// The shadow behind a whole-frame render into the target (k_view_pixels, which writes nothing but frames): the tile id of every cell of
// every env, tile_id's rule once more.  n x 49 bytes against the frames' n x 37.6 / 150.5 KB.
__global__ __launch_bounds__(256) void k_view_ids(const uint8_t* __restrict__ image, int64_t n, const uint8_t* __restrict__ lut, uint8_t* __restrict__ shadow) {
    const int64_t total = n * CELLS;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int cell = (int)(i % CELLS);
        const uint8_t* p = image + i * 3;
        const uint32_t key = ((uint32_t)p[0] | (uint32_t)p[1] << 3 | (uint32_t)p[2] << 6) & 255u;
        shadow[i] = lut[(cell == AGENT_CELL ? 256 : 0) + key];
    }
}
#endif  // __HIPCC__
