// bbai_viewpxn.hpp -- the agent's V x V view as pixels, V in 3, 5, 7, 9, 11 at tile sizes 8, 16 and 32: k_view_pixels_n<V, TS>,
// RGBImgPartialObsWrapper(ViewSizeWrapper(env, V), tile_size).observation of rows of an ENCODED uint8[rows][V][V][3] buffer
// (include/bbai_view_pixels.h bbai_render_view_pixels).  A stand-alone whole-frame render in the shape of k_view_pixels<TS>
// (bbai_viewpx.hpp), with the view size a template parameter next to the tile size; the 7x7 kernels (k_render and its kin at 8,
// k_view_pixels / k_view_delta at 16 / 32) stay what the batch's own pixels are drawn with.
//
// The first part is plain C++ -- a frame's geometry, and which cell and which bytes of its tile every piece of a 16-byte chunk is -- which
// the host tests compile with g++ (tests/test_view_pixels_host.py).  The kernel below it is part of bbai_engine.hip's translation unit:
// included next to bbai_viewpx.hpp, at global scope.  The launch is bbai_engine.hip's (view_pixels_launch).
#pragma once
#include "bbai_types.hpp"

namespace bbai {

constexpr int VIEWPXN_BLOCK = 1024;              // lanes of a block: lane = cell of the item's envs
constexpr int VIEWPXN_ITEM_BYTES = 150528;       // frames of a work item, at most: what k_view_pixels found good (4 frames at 16, one at 32)
constexpr int VIEWPXN_SLICE_MIN = 65536;         // a frame of at least this much is halved once more while there are fewer items than blocks

BB_HD constexpr bool viewpxn_view_ok(int v) { return v == 3 || v == 5 || v == 7 || v == 9 || v == 11; }
BB_HD constexpr bool viewpxn_tile_ok(int ts) { return ts == 8 || ts == 16 || ts == 32; }

// A frame at view size V and tile size TS in memory: V TS pixel rows of 3 V TS bytes, pixel row = view vj, pixel column = view vi (the
// encoding is indexed [vi][vj]: cell = V vi + vj; the agent stands in (V / 2, V - 1)).  It is a flat run of F16 16-byte chunks -- 3 V^2 TS^2
// is a multiple of 64 at every size, so frames start 16-byte aligned -- and a chunk is PPC pieces of P bytes that never cross a tile's
// pixel row: at 8 a tile's pixel row is 24 bytes and a frame's 24 V, an odd multiple of 8, so a chunk is two 8-byte pieces, of two
// tiles or two pixel rows where it straddles (k_render builds its 16 bytes the same way); at 16 / 32 it is one 16-byte piece.
template <int V, int TS> struct ViewPxN {
    static_assert(viewpxn_view_ok(V) && viewpxn_tile_ok(TS), "view sizes 3 .. 11, tile sizes 8 / 16 / 32");
    static constexpr int CELLS = V * V;
    static constexpr int AGENT_CELL = (V / 2) * V + V - 1;           // 5, 14, 27, 44, 65
    static constexpr int ENC_BYTES = 3 * CELLS;                      // an encoded row: 27 .. 363 (odd: byte loads)
    static constexpr int TILE_ROW = TS * 3;                          // a tile's pixel row: 24 / 48 / 96
    static constexpr int TILE_BYTES = TS * TILE_ROW;                 // 192 / 768 / 3072
    static constexpr int ROW_BYTES = V * TILE_ROW;
    static constexpr int BYTES = ROW_BYTES * V * TS;                 // 1 728 (3, 8) .. 371 712 (11, 32)
    static constexpr int F16 = BYTES / 16;                           // 16-byte chunks per frame
    static constexpr int P = TS == 8 ? 8 : 16;                       // bytes per piece
    static constexpr int PPC = 16 / P;                               // pieces per chunk: 2 / 1 / 1
    static constexpr int PPT = TILE_ROW / P;                         // pieces per tile's pixel row: 3 / 3 / 6
    static constexpr int PPR = V * PPT;                              // pieces per pixel row
    static constexpr int MAX_ENVS = VIEWPXN_BLOCK / CELLS;           // envs of a work item at most: 113, 40, 20, 12, 8
    static constexpr bool LDS = TS <= 16;                            // the atlas in LDS (12.5 / 50 KB); at 32 (200 KB) through L2
    static_assert(BYTES % 64 == 0 && TILE_ROW % P == 0 && TILE_BYTES % 16 == 0, "whole chunks per frame, whole pieces per tile row");
};

// Piece h (0 .. PPC - 1) of chunk j (0 .. F16 - 1) of a frame: the view cell it shows and where its P bytes start inside that cell's tile.
struct ViewPxPiece { uint32_t cell, off; };
template <int V, int TS>
BB_HD constexpr ViewPxPiece viewpxn_piece(uint32_t j, uint32_t h) {
    using F = ViewPxN<V, TS>;
    const uint32_t p = j * F::PPC + h;
    const uint32_t py = p / F::PPR, px = p - py * F::PPR;            // pixel row; piece of that row
    const uint32_t tx = px / F::PPT, part = px - tx * F::PPT;        // view vi; piece of the tile's row
    return ViewPxPiece{tx * V + py / TS, (py % TS) * F::TILE_ROW + part * F::P};
}

// The launch shape (view_pixels_launch; babyai_amd/engine.py view_pixels_items restates it for the tests and the bench): work items of at
// most VIEWPXN_ITEM_BYTES of frames -- `envs_per_item` whole frames (never more than the lane = cell phase has lanes for: MAX_ENVS; fewer
// while that still leaves an item per block), or one of `slices` parts of one frame where a frame is larger (V >= 9 at 32), twice as
// many for frames of VIEWPXN_SLICE_MIN bytes or more while there are fewer items than blocks.  One of the two is 1.
struct ViewPxItems { int envs_per_item, slices; int64_t items; };
BB_HD constexpr ViewPxItems viewpxn_items(int view_size, int tile_size, int64_t count, int64_t blocks) {
    const int cells = view_size * view_size;
    const int64_t bytes = (int64_t)3 * cells * tile_size * tile_size;
    int64_t epi = VIEWPXN_ITEM_BYTES / bytes, slices = 1;
    if (epi > VIEWPXN_BLOCK / cells) epi = VIEWPXN_BLOCK / cells;
    if (epi > 1 && count / blocks < epi) epi = count / blocks;
    if (epi < 1) epi = 1;
    if (epi == 1) {
        slices = (bytes + VIEWPXN_ITEM_BYTES - 1) / VIEWPXN_ITEM_BYTES;
        if (bytes >= VIEWPXN_SLICE_MIN && count * slices < blocks) slices *= 2;
    }
    return ViewPxItems{(int)epi, (int)slices, slices > 1 ? count * slices : (count + epi - 1) / epi};
}

}  // namespace bbai

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "bbai_kernels.hpp"
#include "bbai_viewpx.hpp"

using namespace bbai;

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));      // an 8-byte piece (tile size 8)

// ------------------------------------------------------------------------------------------
// k_view_pixels_n : the V x V view of listed rows of an encoded buffer as uint8[V TS][V TS][3] frames (bbai_render_view_pixels)
// ------------------------------------------------------------------------------------------
// k_view_pixels<TS>'s argument record and its four steps per work item, persistent blocks (bbai_viewpx.hpp):
//   1. the item's encodings -- 3 bytes per cell, lane = cell of env tid / V^2 of the item, 3 V^2 contiguous bytes per env -- are ALREADY in
//      registers (viewn_px_fetch): they were loaded while the previous item's stores were issued;
//   2. lane = cell turns them into tile ids in LDS (lut[(cell == AGENT_CELL ? 256 : 0) + key]); ONE barrier (the id planes, a block's
//      lanes each, are double-buffered: the next item's is written while slower waves still read this item's);
//   3. the next item's encodings are requested;
//   4. the frames leave as 16-byte nontemporal stores, VIEWPX_UNROLL chunks per lane in flight, a wave's 64 chunks contiguous (1 KiB);
//      a chunk is viewpxn_piece's one or two pieces of the atlas, every divisor a compile-time constant.
// The atlas is in LDS at 8 and 16, read from global memory / L2 at 32.  Writes nothing but `out`.  A row id outside [0, rows) draws
// every cell with the zero tile the atlas carries behind its last one.  key = (o0 | o1 << 3 | o2 << 6) & 255.
template <int V>
__device__ __forceinline__ uint32_t viewn_px_fetch(const ViewPxArgs& a, int64_t item, int tid) {
    constexpr int C = V * V;
    if (item >= a.items) return VIEWPX_NONE;
    const int64_t first = a.slices > 1 ? item / a.slices : item * a.envs_per_item;
    const int e = tid / C, cell = tid - e * C;
    if (e >= a.envs_per_item || first + e >= a.count) return VIEWPX_NONE;
    const int64_t row = a.ids ? a.ids[first + e] : first + e;
    if (row < 0 || row >= a.rows) return VIEWPX_NONE;
    const uint8_t* p = a.image + row * (3 * C) + cell * 3;
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
}

// chunk j of a frame -> its 16 bytes
template <int V, int TS>
__device__ __forceinline__ u32x4 viewn_px_chunk(const uint8_t* atlas, const uint8_t* ids, uint32_t j) {
    using F = ViewPxN<V, TS>;
    if constexpr (F::PPC == 1) {
        const ViewPxPiece p = viewpxn_piece<V, TS>(j, 0);
        return *(const u32x4*)(atlas + ids[p.cell] * F::TILE_BYTES + p.off);
    } else {
        const ViewPxPiece p = viewpxn_piece<V, TS>(j, 0), q = viewpxn_piece<V, TS>(j, 1);
        const u32x2 lo = *(const u32x2*)(atlas + ids[p.cell] * F::TILE_BYTES + p.off);
        const u32x2 hi = *(const u32x2*)(atlas + ids[q.cell] * F::TILE_BYTES + q.off);
        return u32x4{lo.x, lo.y, hi.x, hi.y};
    }
}

template <int V, int TS>
__global__ __launch_bounds__(VIEWPXN_BLOCK, 8) void k_view_pixels_n(ViewPxArgs a) {      // (8 waves per SIMD: two blocks per CU)
    using F = ViewPxN<V, TS>;
    constexpr uint32_t F16 = F::F16;
    static_assert(VIEWPXN_BLOCK == VIEWPX_BLOCK, "k_view_pixels' launch shape");
    __shared__ __attribute__((aligned(16))) uint8_t s_atlas[F::LDS ? (VIEWPX_MAX_TILES + 1) * F::TILE_BYTES : 16];
    __shared__ __attribute__((aligned(16))) uint8_t s_lut[VIEWPX_LUT_BYTES];
    __shared__ uint8_t s_ids[2][VIEWPXN_BLOCK];           // (envs_per_item * V^2 <= VIEWPXN_BLOCK of a plane are read)
    const int tid = threadIdx.x;
    const uint8_t* atlas = a.atlas;
    if (F::LDS) {
        for (int k = tid; k < (a.n_tiles + 1) * F::TILE_BYTES / 16; k += VIEWPXN_BLOCK) ((u32x4*)s_atlas)[k] = ((const u32x4*)a.atlas)[k];
        atlas = s_atlas;
    }
    if (tid < VIEWPX_LUT_BYTES / 16) ((u32x4*)s_lut)[tid] = ((const u32x4*)a.lut)[tid];
    uint32_t o = viewn_px_fetch<V>(a, blockIdx.x, tid);
    __syncthreads();                                      // atlas and lut loaded
    u32x4* const out = (u32x4*)a.out;
    const int cell = tid % F::CELLS;
    int b = 0;
    for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x, b ^= 1) {
        const int64_t first = a.slices > 1 ? item / a.slices : item * a.envs_per_item;      // first output frame of the item
        const uint32_t slice = (uint32_t)(item - first * a.slices);                         // (0 unless sliced)
        const uint32_t ne = a.slices > 1 ? 1u : (uint32_t)(a.count - first < a.envs_per_item ? a.count - first : a.envs_per_item);
        const uint32_t key = ((o & 255u) | ((o >> 8) & 255u) << 3 | ((o >> 16) & 255u) << 6) & 255u;
        s_ids[b][tid] = o == VIEWPX_NONE ? (uint8_t)a.n_tiles : s_lut[(cell == F::AGENT_CELL ? 256 : 0) + key];
        __syncthreads();                                  // (the one barrier of an item: the other id plane is the next item's)
        o = viewn_px_fetch<V>(a, item + gridDim.x, tid);  // the next item's encodings, under this item's stores
        // chunks [q0, q1) of the item, counted from its first frame's first chunk
        const uint32_t q0 = a.slices > 1 ? slice * F16 / (uint32_t)a.slices : 0u;
        const uint32_t q1 = a.slices > 1 ? (slice + 1) * F16 / (uint32_t)a.slices : ne * F16;
        u32x4* const base = out + first * (int64_t)F16;
        const uint8_t* const ids = s_ids[b];
        for (uint32_t qb = q0 + tid; qb < q1; qb += VIEWPX_UNROLL * VIEWPXN_BLOCK) {
            u32x4 v[VIEWPX_UNROLL];
#pragma unroll
            for (int u = 0; u < VIEWPX_UNROLL; ++u) {
                const uint32_t q = qb + u * VIEWPXN_BLOCK < q1 ? qb + u * VIEWPXN_BLOCK : q1 - 1;   // (past the end: a chunk of the item, not stored)
                const uint32_t e = q / F16, j = q - e * F16;
                v[u] = viewn_px_chunk<V, TS>(atlas, ids + e * F::CELLS, j);
            }
#pragma unroll
            for (int u = 0; u < VIEWPX_UNROLL; ++u)
                if (qb + u * VIEWPXN_BLOCK < q1) __builtin_nontemporal_store(v[u], base + qb + u * VIEWPXN_BLOCK);
        }
    }
}
#endif  // __HIPCC__
