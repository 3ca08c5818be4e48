// bbai_viewpx.hpp -- the agent's 7x7 view as pixels at tile sizes 16 and 32: k_view_pixels<TS>, RGBImgPartialObsWrapper(env, tile_size)
// .observation of rows of an ENCODED observation buffer (bbai_render_view).  Tile size 8 is bbai_render.hpp's (k_render and its kin, with
// the delta render); this is a stand-alone full render in the shape of k_render_grid, with GridTile<TS>'s piece arithmetic.
// Part of bbai_engine.hip's translation unit: included next to bbai_gridk.hpp, at global scope.  The launch is bbai_engine.hip's
// (render_view_launch).
#pragma once
#include <hip/hip_runtime.h>
#include "bbai_types.hpp"
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
