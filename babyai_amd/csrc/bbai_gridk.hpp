// bbai_gridk.hpp -- whole-grid outputs of listed envs: the full-grid picture (k_render_grid<TS>, MiniGridEnv.render('rgb_array')) and the
// fully observable encoding (k_full_obs, FullyObsWrapper.observation), with the work-item shapes and argument structs their launches fill.  The
// per-cell parts are bbai_grid.hpp's (which the host tests compile as well).  Both argument structs open with bbai_kernels.hpp's EnvList,
// and k_full_obs's item loop is built from the pieces that stand next to it there (list_item_load / _park / _store; k_view_obs<V> in
// bbai_viewn.hpp is built from the same ones).
// Part of bbai_engine.hip's translation unit: included where the code stood, at global scope.  The launches are bbai_engine.hip's
// (render_grid_launch, full_launch).
#pragma once
#include <hip/hip_runtime.h>
#include "bbai_types.hpp"
#include "bbai_kernels.hpp"
#include "bbai_grid.hpp"

using namespace bbai;

// ------------------------------------------------------------------------------------------
// k_render_grid : the full-grid picture, MiniGridEnv.render('rgb_array', highlight, tile_size), of listed envs (bbai_render_grid)
// ------------------------------------------------------------------------------------------
// A frame is uint8[H ts][W ts][3] (row = y, as Grid.render lays it out): H x W atlas tiles.  Per work item a block builds the tile-id
// planes of its envs in LDS (bbai_grid.hpp: ONE lut lookup per cell, from the live record -- live_rec, as k_tokens / k_bot -- the pose and
// the highlight mask), then streams the frames as 16-byte nontemporal stores, a frame being a flat run of 16-byte chunks (frame bytes
// are a multiple of 192; row bytes need not be a multiple of 16).  A chunk is made of pieces that never cross a tile row: 8 bytes at
// tile size 8 (24-byte tile rows, as render_chunk), 16 bytes at 16 and 32; per piece one multiply-high divide finds its pixel row and
// tile, then the piece is copied from the atlas -- in LDS at 8 and 16 (25 / 102 KB), from L2 at 32 (≈400 KB: it stays resident).
// Work items (render_grid_launch): several envs per item for small frames, several items per env for large ones; persistent blocks.
// Writes nothing but `out`.  An id outside [0, n) draws every cell with the zero tile the atlas carries behind its last one.
constexpr int GRID_BLOCK = 1024;
constexpr int GRID_MAX_ENVS = 32;                // envs per work item
constexpr int GRID_ID_BYTES = 4096;              // tile ids of one work item
constexpr int GRID_MAX_TILES = 132;              // atlas tiles (+ the zero tile)
constexpr int GRID_UNROLL = 4;                   // 16-byte chunks per lane in flight

template <int TS> struct GridTile {
    static constexpr int P = TS == 8 ? 8 : 16;           // bytes per piece
    static constexpr int PPT = TS * 3 / P;               // pieces per tile row: 3, 3, 6
    static constexpr int BYTES = TS * TS * 3;
    static constexpr bool LDS = TS <= 16;
};

struct GridArgs {
    EnvList list;                // the batch, the listed envs, their frames (bbai_kernels.hpp)
    const uint8_t* atlas;        // [n_tiles + 1][TS][TS][3], the last one all zero
    const uint8_t* lut;          // [2][5][256]
    int n_tiles, highlight;
    int envs_per_item, slices;   // one of them is 1
    int64_t items;
    uint32_t frame16;            // 16-byte chunks per frame
    uint64_t frame_magic;        // 2^32 / frame16 + 1: q / frame16 as a multiply-high (q frame16 < 2^32)
    uint32_t ppr;                // pieces per pixel row
    uint64_t ppr_magic;
};
static_assert(sizeof(GridArgs) == 328 && offsetof(GridArgs, atlas) == 256, "k_render_grid's argument layout");

__device__ __forceinline__ uint32_t grid_div(uint32_t q, uint64_t magic) { return (uint32_t)(((uint64_t)q * magic) >> 32); }

template <int TS>
__device__ __forceinline__ const uint8_t* grid_piece(const uint8_t* atlas, const uint8_t* ids, int W, const GridArgs& a, uint32_t p) {
    using G = GridTile<TS>;
    const uint32_t py = grid_div(p, a.ppr_magic), px = p - py * a.ppr;
    const uint32_t tx = px / G::PPT, part = px - tx * G::PPT;
    const int id = ids[(py / TS) * W + tx];
    return atlas + id * G::BYTES + (py % TS) * (TS * 3) + part * G::P;
}

template <int TS>
__global__ __launch_bounds__(GRID_BLOCK, TS == 16 ? 4 : 8) void k_render_grid(GridArgs a) {      // (8 waves per SIMD: two blocks per CU)
    using G = GridTile<TS>;
    __shared__ __attribute__((aligned(16))) uint8_t s_atlas[G::LDS ? (GRID_MAX_TILES + 1) * G::BYTES : 16];
    __shared__ __attribute__((aligned(16))) uint8_t s_lut[GRID_LUT_BYTES];
    __shared__ uint8_t s_ids[GRID_ID_BYTES];
    __shared__ uint32_t s_hl[GRID_MAX_ENVS][MAX_W];
    __shared__ Hot s_hot[GRID_MAX_ENVS];
    __shared__ const uint8_t* s_rec[GRID_MAX_ENVS];
    const int tid = threadIdx.x;
    const EnvList& l = a.list;
    const uint8_t* atlas = a.atlas;
    if (G::LDS) {
        for (int k = tid; k < (a.n_tiles + 1) * G::BYTES / 16; k += GRID_BLOCK) ((u32x4*)s_atlas)[k] = ((const u32x4*)a.atlas)[k];
        atlas = s_atlas;
    }
    for (int k = tid; k < GRID_LUT_BYTES / 16; k += GRID_BLOCK) ((u32x4*)s_lut)[k] = ((const u32x4*)a.lut)[k];
    const int W = l.c.W, HW = l.c.W * l.c.H;
    const int64_t F16 = a.frame16;
    constexpr int ESTRIDE = GRID_BLOCK / GRID_MAX_ENVS;       // the envs' view work spread over the waves (two envs per wave)
    u32x4* const out = (u32x4*)l.out;
    for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int64_t first = a.slices > 1 ? item / a.slices : item * a.envs_per_item;      // first output frame of the item
        const int slice = (int)(item - first * a.slices);                                   // (0 unless sliced)
        const int ne = a.slices > 1 ? 1 : (int)(l.count - first < a.envs_per_item ? l.count - first : a.envs_per_item);
        __syncthreads();                                  // atlas loaded / the previous item's ids consumed
        if (tid % ESTRIDE == 0 && tid / ESTRIDE < ne) {
            const int e = tid / ESTRIDE;
            const int64_t env = l.ids ? l.ids[first + e] : first + e;
            const uint8_t* rec = nullptr;
            Hot h = {};
            if (env >= 0 && env < l.n) {
                h = l.hots[env];
                rec = live_rec(l.c, l.n, env, (uint8_t*)l.recs, (uint8_t*)l.ring, l.depth, l.ring ? h.slot : 0);
                grid_highlight(l.c, rec, h, s_hl[e]);
            }
            s_hot[e] = h;
            s_rec[e] = rec;
        }
        __syncthreads();
        for (int ci = tid; ci < ne * HW; ci += GRID_BLOCK) {
            const int e = ci / HW, cell = ci - e * HW;
            const int y = cell / W, x = cell - y * W;
            const uint8_t* rec = s_rec[e];
            s_ids[ci] = (uint8_t)(rec ? grid_tile(l.c, rec, s_hot[e], s_lut, a.highlight, s_hl[e], x, y) : a.n_tiles);
        }
        __syncthreads();
        // chunks [q0, q1) of the item, counted from its first frame's first chunk
        const int64_t q0 = a.slices > 1 ? slice * F16 / a.slices : 0;
        const int64_t q1 = a.slices > 1 ? (slice + 1) * F16 / a.slices : ne * F16;
        u32x4* const base = out + first * F16;
        for (int64_t qb = q0 + tid; qb < q1; qb += GRID_UNROLL * GRID_BLOCK) {
            u32x4 v[GRID_UNROLL];
#pragma unroll
            for (int u = 0; u < GRID_UNROLL; ++u) {
                const uint32_t q = (uint32_t)(qb + u * GRID_BLOCK < q1 ? qb + u * GRID_BLOCK : q1 - 1);     // (past the end: a chunk of the item, not stored)
                const uint32_t e = a.slices > 1 ? 0u : grid_div(q, a.frame_magic);
                const uint32_t j = q - e * (uint32_t)F16;
                const uint8_t* ids = s_ids + e * HW;
                if (TS == 8) {
                    const uint64_t lo = *(const uint64_t*)grid_piece<TS>(atlas, ids, W, a, 2 * j);
                    const uint64_t hi = *(const uint64_t*)grid_piece<TS>(atlas, ids, W, a, 2 * j + 1);
                    v[u] = u32x4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
                } else {
                    v[u] = *(const u32x4*)grid_piece<TS>(atlas, ids, W, a, j);
                }
            }
#pragma unroll
            for (int u = 0; u < GRID_UNROLL; ++u)
                if (qb + u * GRID_BLOCK < q1) __builtin_nontemporal_store(v[u], base + qb + u * GRID_BLOCK);
        }
    }
}

// ------------------------------------------------------------------------------------------
// k_full_obs : the fully observable encoding, FullyObsWrapper.observation, of listed envs (bbai_observe_full, bbai_step_full)
// ------------------------------------------------------------------------------------------
// A frame is uint8[W][H][3] (F = 3 W H bytes, indexed [x][y] as grid.encode() is).  Work item = envs_per_item envs; per item a block
//   1. copies the H interior rows of each env's appearance plane (H x ES bytes of the live record -- live_rec: both state layouts) into
//      LDS as dwords, FULL_UNROLL independent loads per lane in flight: ONE memory round trip per item (a load per cell in a loop is one
//      round trip per trip, and it measured 2.1 TB/s);
//   2. writes each cell's 3 bytes (bbai_grid.hpp full_cell, on the LDS rows) into the item's frames in LDS at their [x][y] place;
//   3. stores the item's frames -- ONE contiguous byte range of `out` -- from LDS as 16-byte nontemporal chunks that cross frame boundaries
//      freely (BossLevel: F = 1452, not a multiple of 16).  envs_per_item is a multiple of 16 / gcd(F, 16), so every item starts 16-byte
//      aligned and only the end of the whole output can hold a partial chunk: that tail is stored byte by byte.
// The next item's ids and Hots are loaded into registers while the current one is worked on (the item skeleton: bbai_kernels.hpp,
// list_item_*).  Writes nothing but `out`.  An id outside [0, n) gives an all-zero frame.
constexpr int FULL_BLOCK = 512;
constexpr int FULL_LDS = 24576;               // frame bytes of one work item (3 x 25 x 25 x 16 = 30 000 > this: see full_launch)
constexpr int FULL_APP = 16384;               // appearance rows of one work item
constexpr int FULL_MAX_ENVS = 128;            // envs per work item
constexpr int FULL_BPC = 3;                   // persistent blocks per CU (≈ 43 KB of LDS each)
constexpr int FULL_UNROLL = 8;                // dword loads per lane in flight

struct FullArgs {
    EnvList list;                // the batch, the listed envs, their frames (bbai_kernels.hpp)
    int envs_per_item;
    int64_t items;
    uint64_t hw_magic, w_magic, rd_magic;   // multiply-high divides by W H, W and the dwords of an env's rows (grid_div; q < 2^16)
};
static_assert(sizeof(FullArgs) == 296 && offsetof(FullArgs, envs_per_item) == 256, "k_full_obs's argument layout");

__global__ __launch_bounds__(FULL_BLOCK, 6) void k_full_obs(FullArgs a) {      // (6 waves per SIMD: FULL_BPC blocks per CU)
    __shared__ __attribute__((aligned(16))) uint8_t s_frames[FULL_LDS];
    __shared__ __attribute__((aligned(16))) uint32_t s_app[FULL_APP / 4];
    __shared__ __attribute__((aligned(16))) Hot s_hot[FULL_MAX_ENVS];
    __shared__ const uint8_t* s_rec[FULL_MAX_ENVS];
    const int tid = threadIdx.x;
    const EnvList& l = a.list;
    const int W = l.c.W, H = l.c.H, HW = W * H, F = 3 * HW, ES = l.c.ES;
    const int RD = H * ES / 4;                          // dwords of an env's interior rows (ES: a multiple of 4)
    const int D0 = MARGIN * ES / 4;                     // first dword of the interior rows
    u32x4 h = {0u, 0u, 0u, 0u};
    int64_t item = blockIdx.x;
    int64_t env = item < a.items ? list_item_load(l, item, a.envs_per_item, tid, h) : -1;
    for (; item < a.items; item += gridDim.x) {
        const int64_t first = item * a.envs_per_item;
        const int ne = list_item_envs(l, first, a.envs_per_item);
        __syncthreads();                                  // the previous item's frames are stored
        if (tid < ne) list_item_park(l, tid, env, h, s_hot, s_rec);
        __syncthreads();
        for (int k0 = tid; k0 < ne * RD; k0 += FULL_UNROLL * FULL_BLOCK) {
            uint32_t v[FULL_UNROLL];
#pragma unroll
            for (int u = 0; u < FULL_UNROLL; ++u) {
                const int k = k0 + u * FULL_BLOCK;
                v[u] = 0;
                if (k < ne * RD) {
                    const int e = (int)grid_div((uint32_t)k, a.rd_magic);
                    const uint8_t* rec = s_rec[e];
                    if (rec) v[u] = ((const uint32_t*)rec)[D0 + (k - e * RD)];
                }
            }
#pragma unroll
            for (int u = 0; u < FULL_UNROLL; ++u)
                if (k0 + u * FULL_BLOCK < ne * RD) s_app[k0 + u * FULL_BLOCK] = v[u];
        }
        env = item + gridDim.x < a.items ? list_item_load(l, item + gridDim.x, a.envs_per_item, tid, h) : -1;      // the next item's entries, under this item's work
        __syncthreads();
        for (int ci = tid; ci < ne * HW; ci += FULL_BLOCK) {
            const int e = (int)grid_div((uint32_t)ci, a.hw_magic), cell = ci - e * HW;
            const int y = (int)grid_div((uint32_t)cell, a.w_magic), x = cell - y * W;
            uint8_t* o = s_frames + e * F + (x * H + y) * 3;
            if (s_rec[e]) full_cell_key(((const uint8_t*)s_app)[e * RD * 4 + y * ES + x + MARGIN], s_hot[e], x, y, o);
            else o[0] = o[1] = o[2] = 0;
        }
        __syncthreads();
        list_item_store<FULL_BLOCK>(l.out + first * F, s_frames, ne * F, tid);       // 16-byte aligned (see above)
    }
}
