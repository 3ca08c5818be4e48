// bbai_griddelta.hpp -- the full-grid picture of the WHOLE batch into the registered grid target, storing only what changed:
// k_grid_delta<TS> (bbai_render_grid_target, bbai_step_grid_target: include/bbai_grid_target.h), and k_grid_ids, which writes every tile id
// behind a whole-frame render (k_render_grid<TS>, unchanged) while the target's history is not valid.  The record, the planner and the
// geometry of the 64-byte pieces are bbai_gridtarget.hpp's (plain C++: the host tests compile them); the per-cell rule is bbai_grid.hpp's
// (grid_tile / grid_tile_key, highlight = 0: RGBImgObsWrapper draws render('rgb_array', highlight=False)); a 16-byte chunk is built by
// k_render_grid's own rule (grid_piece<TS>, bbai_gridk.hpp).
// Part of bbai_engine.hip's translation unit, included behind bbai_gridk.hpp at global scope.  The launches are bbai_engine.hip's
// (grid_target_launch).
#pragma once
#include <hip/hip_runtime.h>
#include "bbai_types.hpp"
#include "bbai_kernels.hpp"
#include "bbai_grid.hpp"
#include "bbai_gridk.hpp"
#include "bbai_gridtarget.hpp"

using namespace bbai;

// ------------------------------------------------------------------------------------------
// k_grid_delta : every env's frame into the registered buffer, only the 64-byte pieces that hold a changed cell
// ------------------------------------------------------------------------------------------
// The registered buffer holds the previous frame of every env, the shadow the tile id of every cell of it (uint8[n][W H]).  A cell whose
// id is unchanged has unchanged bytes, so only the pieces that hold bytes of a changed cell are stored.  Persistent blocks over static
// groups of G envs (grid_target_launch: as many as the planes below hold); per group
//   A  the H record rows of every env, loaded as dwords a group AHEAD into registers (with the old ids, a byte per lane), go to LDS;
//      lane = cell computes the new id (grid_tile_key on the staged byte), keeps it in the LDS id plane, and where it differs from the
//      old one writes it back to the shadow and sets the cell's bit in the env's per-tile-row mask of dirty columns (an LDS atomic: a
//      turn dirties one cell, a move two, and most env-steps none);
//   barrier; the next group's rows and old ids are requested (they ride under this group's stores), and the Hots of the group after;
//   B  a wave per env lists the tile rows with a non-zero mask -- a tile row is 3 W TS^2 bytes, a whole number of pieces, so a piece
//      lies in ONE tile row (bbai_gridtarget.hpp) and only the pieces [grid_row_first(y), grid_row_first(y + 1)) of a listed row y can
//      be dirty; barrier; the block's waves take the listed rows in turn, four lanes per candidate piece: grid_piece_dirty
//      (grid_piece_segments against the masks) judges it, and a dirty one leaves as four 16-byte nontemporal stores of
//      grid_piece<TS>'s bytes.  Every piece is judged in one place and stored at most once; a reset env (every piece dirty) is H
//      listed rows shared by all waves; a group where nothing changed costs its loads and the barriers.
// The atlas is read through L2 at every tile size: a typical group stores a few hundred bytes, and copying 25 - 400 KB of atlas into
// LDS per block would cost more than that.  Writes the shadow (changed ids) and the dirty pieces of `out`, nothing else.
// (The block size, the planes' sizes and the group arithmetic -- GRIDDELTA_*, griddelta_group, griddelta_shape -- are bbai_gridtarget.hpp's:
// plain C++, so that the host test holds every level's grid against them.)
constexpr int GRIDDELTA_WAVES = GRIDDELTA_BLOCK / 64;

struct GridDeltaArgs {
    GridArgs g;                  // k_render_grid's record: the batch (list.ids NULL, list.count = n, list.out = the registered buffer), the atlas, the lut, grid_piece's divide
    uint8_t* shadow;             // [n][W H]
    GridGeom geom;               // the pieces of a frame (bbai_gridtarget.hpp)
    int envs_per_group;
    int64_t groups;
    uint64_t hw_magic, w_magic, rd_magic;   // multiply-high divides by W H, W and the dwords of an env's rows (grid_div; q < 2^16)
};

template <int TS>
__global__ __launch_bounds__(GRIDDELTA_BLOCK, 4) void k_grid_delta(GridDeltaArgs a) {      // (4 waves per SIMD: two blocks per CU)
    constexpr int T = GRIDDELTA_BLOCK, NW = GRIDDELTA_WAVES, GM = GRIDDELTA_MAX_ENVS;
    __shared__ __attribute__((aligned(16))) uint8_t s_lut[GRID_LUT_BYTES];
    __shared__ __attribute__((aligned(16))) uint32_t s_app[GRIDDELTA_APP];
    __shared__ __attribute__((aligned(16))) uint8_t s_ids[GRIDDELTA_IDS];
    __shared__ __attribute__((aligned(16))) Hot s_hot[2][GM];
    __shared__ const uint8_t* s_rec[2][GM];
    __shared__ uint32_t s_mask[GM][MAX_W + 1];           // [e][y] bit x = cell (x, y) changed
    __shared__ uint32_t s_first[MAX_W + 1];              // grid_row_first(y)
    __shared__ uint16_t s_scan[GM * MAX_W];              // listed rows: e * 32 + y
    __shared__ uint32_t s_nscan;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const EnvList& l = a.g.list;
    const GridGeom& geom = a.geom;
    const int W = l.c.W, H = l.c.H, HW = W * H, ES = l.c.ES, G = a.envs_per_group;
    const int RD = H * ES / 4;                          // dwords of an env's interior rows (ES: a multiple of 4)
    const int D0 = MARGIN * ES / 4;                     // first dword of the interior rows
    const int64_t F16 = a.g.frame16;
    const int64_t stride = gridDim.x;
    for (int k = tid; k < GRID_LUT_BYTES / 16; k += T) ((u32x4*)s_lut)[k] = ((const u32x4*)a.g.lut)[k];
    if (tid <= H) s_first[tid] = grid_row_first(geom, tid);

    // the Hot of this lane's env of group `grp` (lanes < G), loaded two groups ahead
    u32x4 h = {0u, 0u, 0u, 0u};
    int64_t env = -1;
    auto load_hot = [&](int64_t grp) {
        env = -1;
        if (grp < a.groups && tid < G && grp * G + tid < l.n) list_entry(l, grp * G + tid, env, h);
    };
    auto park = [&](int b) {
        if (tid < G) { ((u32x4*)s_hot[b])[tid] = h; s_rec[b][tid] = list_rec(l, env, h); }
    };
    // phase A's inputs of group `grp`, loaded one group ahead: the record rows as dwords, the old id of each of this lane's cells
    uint32_t v[GRIDDELTA_ROW_UNROLL];
    uint32_t old[GRIDDELTA_ID_UNROLL / 4];              // (four ids to a register)
    auto load_rows = [&](int64_t grp, int b) {
        const int64_t env0 = grp * G;
        const int ne = grp < a.groups ? (int)(l.n - env0 < G ? l.n - env0 : G) : 0;
#pragma unroll
        for (int u = 0; u < GRIDDELTA_ROW_UNROLL; ++u) {
            const int k = tid + u * T;
            v[u] = 0;
            if (k < ne * RD) {
                const int e = (int)grid_div((uint32_t)k, a.rd_magic);
                const uint8_t* rec = s_rec[b][e];
                if (rec) v[u] = ((const uint32_t*)rec)[D0 + (k - e * RD)];
            }
        }
#pragma unroll
        for (int u = 0; u < GRIDDELTA_ID_UNROLL / 4; ++u) old[u] = 0;
#pragma unroll
        for (int u = 0; u < GRIDDELTA_ID_UNROLL; ++u) {
            const int ci = tid + u * T;
            if (ci < ne * HW) old[u >> 2] |= (uint32_t)a.shadow[env0 * HW + ci] << (8 * (u & 3));
        }
    };

    int64_t g = blockIdx.x;
    int b = 0;
    load_hot(g);
    park(0);
    __syncthreads();                                      // lut, piece table and the first group's records parked
    load_rows(g, 0);
    load_hot(g + stride);
    for (; g < a.groups; g += stride, b ^= 1) {
        const int64_t env0 = g * G;
        const int ne = (int)(l.n - env0 < G ? l.n - env0 : G);
        __syncthreads();                                  // the previous group's ids, masks and list are read
#pragma unroll
        for (int u = 0; u < GRIDDELTA_ROW_UNROLL; ++u)
            if (tid + u * T < ne * RD) s_app[tid + u * T] = v[u];
        park(b ^ 1);                                      // the next group's
        for (int k = tid; k < G * (MAX_W + 1); k += T) (&s_mask[0][0])[k] = 0;
        if (tid == 0) s_nscan = 0;
        __syncthreads();
        // A: new ids, dirty-column masks, shadow write-back
#pragma unroll
        for (int u = 0; u < GRIDDELTA_ID_UNROLL; ++u) {
            const int ci = tid + u * T;
            if (ci < ne * HW) {
                const int e = (int)grid_div((uint32_t)ci, a.hw_magic), cell = ci - e * HW;
                const int y = (int)grid_div((uint32_t)cell, a.w_magic), x = cell - y * W;
                const int key = ((const uint8_t*)s_app)[e * RD * 4 + y * ES + x + MARGIN];
                const uint8_t id = (uint8_t)grid_tile_key(key, s_hot[b][e], s_lut, x, y);
                s_ids[ci] = id;
                if (id != (uint8_t)(old[u >> 2] >> (8 * (u & 3)))) {
                    a.shadow[env0 * HW + ci] = id;
                    atomicOr(&s_mask[e][y], 1u << x);
                }
            }
        }
        __syncthreads();
        load_rows(g + stride, b ^ 1);                     // the next group's inputs ride under this group's stores
        load_hot(g + 2 * stride);
        // B: the rows that own candidate pieces
        for (int e = wave; e < ne; e += NW) {
            const bool need = lane < H && s_mask[e][lane < H ? lane : 0] != 0;
            const uint64_t m = __ballot(need);
            if (!m) continue;
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&s_nscan, (uint32_t)__builtin_popcountll(m));
            base = (uint32_t)__shfl((int)base, 0);
            if (need) s_scan[base + __builtin_popcountll(m & ((1ull << lane) - 1))] = (uint16_t)(e * 32 + lane);
        }
        __syncthreads();
        const uint32_t nscan = s_nscan;
        for (uint32_t k = wave; k < nscan; k += NW) {
            const uint32_t entry = s_scan[k];
            const int e = (int)(entry >> 5), y = (int)(entry & 31u);
            const uint32_t c1 = s_first[y + 1] * 4;
            const uint8_t* ids = s_ids + e * HW;
            u32x4* const base = (u32x4*)l.out + (env0 + e) * F16;
            for (uint32_t c = s_first[y] * 4 + lane; c < c1; c += 64) {      // chunk c of the frame: piece c / 4
                if (!grid_piece_dirty(geom, c >> 2, s_mask[e])) continue;
                u32x4 val;
                if (TS == 8) {
                    const uint64_t lo = *(const uint64_t*)grid_piece<TS>(a.g.atlas, ids, W, a.g, 2 * c);
                    const uint64_t hi = *(const uint64_t*)grid_piece<TS>(a.g.atlas, ids, W, a.g, 2 * c + 1);
                    val = u32x4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
                } else {
                    val = *(const u32x4*)grid_piece<TS>(a.g.atlas, ids, W, a.g, c);
                }
                __builtin_nontemporal_store(val, base + c);
            }
        }
    }
}

// The shadow behind a whole-frame render into the target (k_render_grid, which writes nothing but frames): the tile id of every cell of
// every env, by grid_tile with highlight = 0.  n x W H bytes against the frames' n x 3 W H ts^2.
__global__ __launch_bounds__(256) void k_grid_ids(EnvList l, const uint8_t* __restrict__ lut, uint8_t* __restrict__ shadow) {
    const int W = l.c.W, HW = l.c.W * l.c.H;
    const int64_t total = l.n * HW;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t env = i / HW;
        const int cell = (int)(i - env * HW), y = cell / W, x = cell - y * W;
        const Hot h = l.hots[env];
        const uint8_t* rec = live_rec(l.c, l.n, env, (uint8_t*)l.recs, (uint8_t*)l.ring, l.depth, l.ring ? h.slot : 0);
        shadow[i] = (uint8_t)grid_tile(l.c, rec, h, lut, 0, nullptr, x, y);
    }
}
