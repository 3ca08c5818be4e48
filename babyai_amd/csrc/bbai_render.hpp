// bbai_render.hpp -- the partial-view pixel render (RGBImgPartialObsWrapper as a tile-atlas gather): the full render (k_render, k_render_q),
// the delta render into the registered target (k_render_delta) and its store-only form behind a step that found the dirty cells itself
// (k_render_dstore; k_render_dstore_lw: its 64-byte pieces from a ticket queue).  Every stage the kernels share is written once: load_atlas_lds / load_lut_lds, tile_id, store_chunk16, delta_cell,
// init_line_table, list_dirty_lines, store_listed_lines, init_piece_cells, init_chunk_table, store_chunk16_t, store_dirty_pieces.  The piece
// stores address their chunks through a per-block table (chunk_recipe below: the frame geometry of a 16-byte chunk, worked out once per
// block and not once per store); the full renders keep the arithmetic form (render_chunk).  Two copies remain, each marked where it
// stands, because the shared form changed the compiler's register counts: phase A in k_render_delta's piece branch, B1 in k_render_dstore.
//
// The first part is plain C++ -- the geometry of a frame in memory, which the host tests read through tests/hostsim (hs_line_cells).  The
// kernels below it are part of bbai_engine.hip's translation unit: they are included where they stood and stay at global scope (u32x4, CELLS
// and AGENT_CELL come from bbai_kernels.hpp) -- the resource report, bench.py and tools/summarize_profile.py find them by their bare names.  The launches
// are bbai_engine.hip's (render_launch).
#pragma once
#include "bbai_types.hpp"

namespace bbai {

constexpr int RENDER_QUEUE_DEFAULT = 1;         // queue shape of render_launch used from RENDER_QUEUE_MIN_ENVS up
constexpr int RENDER_QUEUE_PACED = 3;           // ... with time-paced tickets: (1024, 8) blocks, two interleaved counters
constexpr int64_t RENDER_QUEUE_MIN_ENVS = 262144;

constexpr int CHUNKS_PER_ROW = PIX * 3 / 8;       // 21 eight-byte chunks per pixel row
constexpr int VEC_PER_ENV = PIX_BYTES / 16;       // 588 sixteen-byte stores per env

// The delta render's units (k_render_delta below has the whole picture)
constexpr int LINE_BYTES = 128;
constexpr int DELTA_UNIT = 8;                                          // envs per line-aligned unit
constexpr int UNIT_LINES = DELTA_UNIT * PIX_BYTES / LINE_BYTES;        // 588
static_assert(DELTA_UNIT * PIX_BYTES % LINE_BYTES == 0 && PIX_BYTES % 64 == 0, "8-env units are whole 128-byte lines");
constexpr int RENDER_PIECE_DEFAULT = 64;                               // option "render_piece_bytes" (render_launch)

// The cells of one env that bytes [s, t) of its 56x56x3 image come from (s, t multiples of 8: one 8-byte chunk per tile row piece).
BB_HD uint64_t line_cells(int s, int t) {
    uint64_t m = 0;
    for (int b = s; b < t; b += 8) {
        const int ch = b >> 3, py = ch / CHUNKS_PER_ROW, cx = ch - py * CHUNKS_PER_ROW;
        m |= 1ull << ((cx / 3) * VIEW + (py >> 3));
    }
    return m;
}

// The recipe of the 16-byte chunk k (of VEC_PER_ENV) of an env's image: its two 8-byte halves (chunks 2k and 2k + 1 of render_chunk) as
// (view cell, byte offset inside the atlas tile = row in tile * 24 + third of the row * 8), packed one byte each: cell A, offset A, cell B,
// offset B from the low byte up.  It depends on the chunk's place in the frame alone: the piece stores read it from a table in LDS
// (init_chunk_table) where the full renders redo the divisions per store.  Worked out from the byte address, not from render_chunk's
// chunk arithmetic -- the assertion below holds the two against each other for every chunk.
BB_HD constexpr uint32_t chunk_half_recipe(int byte) {
    const int row = byte / (PIX * 3), xb = byte - row * (PIX * 3);        // pixel row of the frame, byte within the row
    const int cell = xb / (TILE * 3) * VIEW + row / TILE;                  // view cell: column * VIEW + row (as tile_id's `cell`)
    const int off = row % TILE * (TILE * 3) + xb % (TILE * 3);             // byte inside the tile
    return (uint32_t)cell | (uint32_t)off << 8;
}
BB_HD constexpr uint32_t chunk_recipe(int k) { return chunk_half_recipe(16 * k) | chunk_half_recipe(16 * k + 8) << 16; }

// ... against render_chunk's arithmetic, restated (render_chunk reads LDS and is no constant expression)
BB_HD constexpr bool chunk_recipes_match_render_chunk() {
    for (int k = 0; k < VEC_PER_ENV; ++k) {
        uint32_t w = 0;
        for (int h = 0; h < 2; ++h) {
            const int ch = 2 * k + h;
            const int py = ch / CHUNKS_PER_ROW, cx = ch - py * CHUNKS_PER_ROW;
            const int ti = cx / 3, part = cx - ti * 3;
            const int tj = py >> 3, ty = py & 7;
            const int cell = ti * VIEW + tj, off = ty * 24 + part * 8;
            if (cell < 0 || cell >= VIEW * VIEW || off < 0 || off + 8 > TILE_BYTES) return false;
            w |= ((uint32_t)cell | (uint32_t)off << 8) << (16 * h);
        }
        if (chunk_recipe(k) != w) return false;
    }
    return true;
}
static_assert(TILE == 8 && TILE_BYTES <= 256 && VIEW * VIEW <= 256, "a cell and a tile offset fit a byte each");
static_assert(chunk_recipes_match_render_chunk(), "chunk_recipe(k) = render_chunk's (cell, offset) of chunks 2k and 2k + 1, for every k");

// P-byte pieces of an env's image (store_dirty_pieces below)
template <int P>
struct Pieces {
    static_assert(P == 16 || P == 32 || P == 64, "pieces of 16, 32 or 64 bytes");
    static_assert(PIX_BYTES % P == 0, "whole pieces per env");
    static constexpr int NP = PIX_BYTES / P;          // pieces per env (147 at P = 64)
    static constexpr int S = P / 16;                  // 16-byte stores per piece
};

}  // namespace bbai

#if defined(__HIPCC__)
#include "bbai_kernels.hpp"

using namespace bbai;

// ------------------------------------------------------------------------------------------
// k_render : encoded obs -> 56x56x3 pixels through the tile atlas
// ------------------------------------------------------------------------------------------
// The atlas (8-byte words) and the 512-byte lut (lut[256 * agent's cell + key]) into a block's LDS; the caller's barrier makes them visible.
__device__ __forceinline__ void load_atlas_lds(uint8_t* s_atlas, const uint8_t* atlas, int n_tiles, int tid, int T) {
    for (int k = tid; k < n_tiles * TILE_BYTES / 8; k += T) ((uint64_t*)s_atlas)[k] = ((const uint64_t*)atlas)[k];
}
__device__ __forceinline__ void load_lut_lds(uint8_t* s_lut, const uint8_t* lut, int tid, int T) {
    for (int k = tid; k < 512; k += T) s_lut[k] = lut[k];
}

// The atlas tile of view cell `cell` whose encoding is (o0, o1, o2); the agent's cell has a table of its own.
__device__ __forceinline__ uint8_t tile_id(const uint8_t* s_lut, int o0, int o1, int o2, int cell) {
    const int key = o0 | (o1 << 3) | (o2 << 6);
    return s_lut[(cell == AGENT_CELL ? 256 : 0) + key];
}

// One 8-byte piece of the env's pixel image: chunk id -> (tile, row in tile, third of the row).
__device__ __forceinline__ uint64_t render_chunk(const uint8_t* s_atlas, const uint8_t* tiles49, int ch) {
    const int py = ch / CHUNKS_PER_ROW, cx = ch - py * CHUNKS_PER_ROW;
    const int ti = cx / 3, part = cx - ti * 3;        // tile column (view x), 8-byte third of the tile row
    const int tj = py >> 3, ty = py & 7;              // tile row (view y), row inside the tile
    const int tile = tiles49[ti * VIEW + tj];
    return *(const uint64_t*)(s_atlas + tile * TILE_BYTES + ty * 24 + part * 8);
}

// The 16-byte chunk k (of VEC_PER_ENV) of the env whose tile ids are `t49`, stored to `dst`.  Streaming output: kept out of L2 / MALL.
__device__ __forceinline__ void store_chunk16(const uint8_t* s_atlas, const uint8_t* t49, int k, u32x4* dst) {
    const uint64_t lo = render_chunk(s_atlas, t49, 2 * k);
    const uint64_t hi = render_chunk(s_atlas, t49, 2 * k + 1);
    u32x4 v = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
    __builtin_nontemporal_store(v, dst);
}

// The same store through the chunk table (`s_ct`: chunk_recipe of every chunk, init_chunk_table): one table word, two tile ids, two atlas
// words -- no division per store.  The same bytes as store_chunk16.
__device__ __forceinline__ void init_chunk_table(uint32_t* s_ct, int tid, int T) {
    for (int k = tid; k < bbai::VEC_PER_ENV; k += T) s_ct[k] = bbai::chunk_recipe(k);
}
__device__ __forceinline__ void store_chunk16_t(const uint8_t* s_atlas, const uint32_t* s_ct, const uint8_t* t49, int k, u32x4* dst) {
    const uint32_t w = s_ct[k];
    const uint32_t ta = t49[w & 0xff], tb = t49[(w >> 16) & 0xff];
    const uint64_t lo = *(const uint64_t*)(s_atlas + ta * TILE_BYTES + ((w >> 8) & 0xff));
    const uint64_t hi = *(const uint64_t*)(s_atlas + tb * TILE_BYTES + (w >> 24));
    u32x4 v = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
    __builtin_nontemporal_store(v, dst);
}

// (Round 3's alternative input -- a fused tile plane, one masked appearance byte per cell, left behind by k_step -- was measured
// once more with the ticket queue in round 4 (profiles/r04/render_queue_counters_1M_lease_d.jsonl: k_render 1.503 vs 1.505 ms, k_step
// + 0.02 ms) and removed.)
template <int RENDER_GROUP, int RENDER_BLOCK>     // envs per block iteration (between two barriers); threads per block
__global__ __launch_bounds__(RENDER_BLOCK) void k_render(int64_t n, const uint8_t* __restrict__ image,
                                                         uint8_t* __restrict__ pixels, const uint8_t* __restrict__ atlas,
                                                         const uint8_t* __restrict__ lut, int n_tiles,
                                                         uint8_t* __restrict__ shadow /* NULL, or the registered target's tile ids [n][49] (k_render_delta) */) {
    __shared__ __attribute__((aligned(16))) uint8_t s_atlas[MAX_TILES * TILE_BYTES];
    __shared__ uint8_t s_lut[512];
    __shared__ uint8_t s_tile[RENDER_GROUP * VIEW * VIEW + 8];
    load_atlas_lds(s_atlas, atlas, n_tiles, threadIdx.x, RENDER_BLOCK);
    load_lut_lds(s_lut, lut, threadIdx.x, RENDER_BLOCK);
    const int64_t ngroups = (n + RENDER_GROUP - 1) / RENDER_GROUP;
    for (int64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int64_t env0 = grp * RENDER_GROUP;
        const int ne = (int)(n - env0 < RENDER_GROUP ? n - env0 : RENDER_GROUP);
        __syncthreads();                               // atlas loaded / previous group's tiles consumed
        // encoded cell -> atlas tile, once per cell (49 per env)
        for (int c = threadIdx.x; c < ne * VIEW * VIEW; c += RENDER_BLOCK) {
            const int e = c / (VIEW * VIEW), cell = c - e * (VIEW * VIEW);
            const uint8_t* o = image + (env0 + e) * OBS_BYTES + cell * 3;
            s_tile[c] = tile_id(s_lut, o[0], o[1], o[2], cell);
            if (shadow) shadow[env0 * (VIEW * VIEW) + c] = s_tile[c];
        }
        __syncthreads();
        // 16 bytes per lane per store: a wave writes 1 KiB of contiguous pixels
        u32x4* out = (u32x4*)(pixels + env0 * PIX_BYTES);
        for (int q = threadIdx.x; q < ne * VEC_PER_ENV; q += RENDER_BLOCK) {
            const int e = q / VEC_PER_ENV, k = q - e * VEC_PER_ENV;
            store_chunk16(s_atlas, s_tile + e * (VIEW * VIEW), k, out + q);
        }
    }
}

// k_render_q: the same render from PERSISTENT blocks (the atlas is loaded into LDS once per block) that take their work from an
// atomic ticket counter, so that the chip's stores advance through the output as ONE compact, evenly paced window -- the order
// in which the pure store stream is fastest (render_launch has the measurements).
//   * a ticket = K consecutive G-env groups; the next ticket is taken while the first group of the current one is being
//     staged, so its latency rides under the stores;
//   * NC counters, 256 bytes apart, INTERLEAVED: ticket t of counter c is super-group t * NC + c, a block uses counter
//     blockIdx % NC (= its XCD for NC = 8).  Shipped: NC = 1, K = 1 -- more counters or bigger tickets relieve the ticket rate
//     (~88 M/s per address) and measure SLOWER: the counters drift apart, the window widens;
//   * the counters clean up after themselves: the last block to leave (a departure counter) zeroes them for the next launch,
//     so the step path carries no memset.
// Tile rows and tickets are double-buffered: one barrier per group.
// (The counters are the handle's: two renders of one handle never overlap -- every entry point orders a call on another stream behind the
// handle's previous call, enter_call -- and a launch that was aborted by a device fault leaves a handle that is unusable anyway.)
template <int RENDER_GROUP, int RENDER_BLOCK, int NC, int K>
__global__ __launch_bounds__(RENDER_BLOCK) void k_render_q(int64_t n, const uint8_t* __restrict__ image,
                                                           uint8_t* __restrict__ pixels, const uint8_t* __restrict__ atlas,
                                                           const uint8_t* __restrict__ lut, int n_tiles, unsigned int* __restrict__ counters,
                                                           int pace_x16 /* experiment: 0, or 1/16 ns of wall clock per ticket (render_launch) */,
                                                           uint8_t* __restrict__ shadow /* NULL, or the registered target's tile ids [n][49] (k_render_delta) */) {
    __shared__ __attribute__((aligned(16))) uint8_t s_atlas[MAX_TILES * TILE_BYTES];
    __shared__ uint8_t s_lut[512];
    __shared__ uint8_t s_tile[2][RENDER_GROUP * VIEW * VIEW + 8];
    __shared__ unsigned int s_ticket[2];
    __shared__ unsigned long long s_origin;
    load_atlas_lds(s_atlas, atlas, n_tiles, threadIdx.x, RENDER_BLOCK);
    load_lut_lds(s_lut, lut, threadIdx.x, RENDER_BLOCK);
    const int64_t all_groups = (n + RENDER_GROUP - 1) / RENDER_GROUP;
    const int64_t n_super = (all_groups + K - 1) / K;
    const unsigned int cidx = blockIdx.x % NC;
    unsigned int* counter = counters + 64 * cidx;
    int buf = 0, tp = 0;
    if (threadIdx.x == 0) {
        const unsigned int t0 = atomicAdd(counter, 1u);
        s_ticket[0] = t0;
        // time-paced tickets (experiment): ticket sg is not started before origin + sg x pace; the 100-MHz constant clock in 1/16 ns
        s_origin = __builtin_amdgcn_s_memrealtime() * 160ull - ((unsigned long long)t0 * NC + cidx) * (unsigned long long)pace_x16;
    }
    __syncthreads();
    for (;;) {
        const int64_t sg = (int64_t)s_ticket[tp] * NC + cidx;
        if (sg >= n_super) break;
        if (pace_x16) {
            const unsigned long long due = s_origin + (unsigned long long)sg * (unsigned long long)pace_x16;
            while (__builtin_amdgcn_s_memrealtime() * 160ull < due) __builtin_amdgcn_s_sleep(1);
        }
#pragma unroll
        for (int kk = 0; kk < K; ++kk) {
            const int64_t grp = sg * K + kk;
            if (grp >= all_groups) break;
            const int64_t env0 = grp * RENDER_GROUP;
            const int ne = (int)(n - env0 < RENDER_GROUP ? n - env0 : RENDER_GROUP);
            for (int c = threadIdx.x; c < ne * VIEW * VIEW; c += RENDER_BLOCK) {
                const int e = c / (VIEW * VIEW), cell = c - e * (VIEW * VIEW);
                const uint8_t* o = image + (env0 + e) * OBS_BYTES + cell * 3;
                s_tile[buf][c] = tile_id(s_lut, o[0], o[1], o[2], cell);
                if (shadow) shadow[env0 * (VIEW * VIEW) + c] = s_tile[buf][c];
            }
            if (kk == 0 && threadIdx.x == 0) s_ticket[tp ^ 1] = atomicAdd(counter, 1u);      // the next ticket rides under this one's stores
            __syncthreads();
            u32x4* out = (u32x4*)(pixels + env0 * PIX_BYTES);
            for (int q = threadIdx.x; q < ne * VEC_PER_ENV; q += RENDER_BLOCK) {
                const int e = q / VEC_PER_ENV, k = q - e * VEC_PER_ENV;
                store_chunk16(s_atlas, s_tile[buf] + e * (VIEW * VIEW), k, out + q);
            }
            buf ^= 1;
        }
        tp ^= 1;
    }
    // every block has taken its last ticket before it arrives here (the failing ticket was read through LDS behind a barrier);
    // the last one to arrive leaves all counters at zero for the next launch
    if (threadIdx.x == 0) {
        unsigned int* departed = counters + 64 * NC;
        if (atomicAdd(departed, 1u) == gridDim.x - 1) {
            for (int c = 0; c <= NC; ++c) atomicExch(counters + 64 * c, 0u);
        }
    }
}

// ---- delta render into the registered target (bbai_set_render_target) ----------------------------------------------------------
// The registered buffer holds the previous frame of every env, and the handle's shadow plane holds the atlas tile id of every cell
// of that frame (uint8[n][49]).  A frame cell whose tile id is unchanged has unchanged bytes, so only the parts of the frame that
// touch a changed cell are stored: 64-byte pieces by default (render_piece_bytes; store_dirty_pieces below), or, with the option at
// 128, whole 128-byte lines -- the line form this paragraph describes.  8 envs are 8 x 9408 = 588 x 128 bytes: a unit of 8 envs
// starts on a line boundary whenever the buffer does (render_launch checks the alignment), and a line belongs to one unit; inside
// it a line touches one env or two (9408 = 73.5 lines).  Per G-env group of a block iteration:
//   A   one wave per env, one lane per cell: the new tile id (s_lut, as k_render), its old id from the shadow, a ballot gives the
//       env's 49-bit dirty mask; the changed cells' ids go back to the shadow;
//   B1  one lane per line: (dirty mask of its env(s)) & (the cells the line touches: a per-block table) -> a compacted line list;
//   B2  8 lanes per listed line, 16 bytes each (render_chunk, as k_render): one full 128-byte line per 8 lanes.
// Work is assigned statically (no ticket counter: one counter serves ~88 M tickets/s, which is the full render's own time at
// 8-env tickets), so the next group's encoding and shadow bytes are loaded before the current group's stores.  SCHED 0: block b
// takes groups b, b + grid, ... (the chip's stores advance as one window); 1: a contiguous range of groups per block.
// Tables and tiles are double-buffered: two barriers per group.  While the shadow is not valid, render_launch runs the full render
// (k_render_q / k_render) instead, which writes every byte and, given the shadow, every tile id.
// (LINE_BYTES, DELTA_UNIT, UNIT_LINES and line_cells: the plain C++ at the top of this file.)

// A for one env: the lane's cell gets its new tile id (dead lanes: none), which goes to the env's ids in LDS (`t49`) and, where it differs
// from `old`, back to the env's shadow row.  Returns the env's dirty mask (a ballot: the whole wave calls).
__device__ __forceinline__ uint64_t delta_cell(const uint8_t* s_lut, uint32_t o0, uint32_t o1, uint32_t o2, uint32_t old, bool live, int lane,
                                               uint8_t* t49, uint8_t* shadow_row) {
    const uint32_t id = live ? tile_id(s_lut, o0, o1, o2, lane) : 0;
    const bool d = live && id != old;
    const uint64_t m = __ballot(d);
    if (live) t49[lane] = (uint8_t)id;
    if (d) shadow_row[lane] = (uint8_t)id;
    return m;
}

// The line table of a unit: a line's first env in the unit (s_lea), the cells it draws from that env (s_lma) and from the next one
// (s_lmb; 0: the line lies inside one env).
__device__ __forceinline__ void init_line_table(uint8_t* s_lea, uint64_t* s_lma, uint64_t* s_lmb, int tid, int T) {
    for (int l = tid; l < UNIT_LINES; l += T) {
        const int b0 = l * LINE_BYTES, b1 = b0 + LINE_BYTES;
        const int ea = b0 / PIX_BYTES, eb = (b1 - 1) / PIX_BYTES;
        s_lea[l] = (uint8_t)ea;
        s_lma[l] = line_cells(b0 - ea * PIX_BYTES, (eb != ea ? (ea + 1) * PIX_BYTES : b1) - ea * PIX_BYTES);
        s_lmb[l] = eb != ea ? line_cells(0, b1 - eb * PIX_BYTES) : 0;
    }
}

// B1: the dirty ones of a group's `nl` lines as a list (any order: every listed line is stored whole, by 8 lanes).  `dmask`: the group's
// dirty masks per env; `nd`: the list's length, zeroed behind a barrier before the call.  One LDS atomic per wave that has a dirty line.
__device__ __forceinline__ void list_dirty_lines(const uint64_t* dmask, const uint8_t* s_lea, const uint64_t* s_lma, const uint64_t* s_lmb,
                                                 uint16_t* list, unsigned int* nd, int nl, int tid, int T) {
    const int lane = tid & 63;
    for (int L0 = tid - lane; L0 < nl; L0 += T) {                      // (whole waves: the ballot below)
        const int L = L0 + lane;
        bool d = false;
        if (L < nl) {
            const int u = L / UNIT_LINES, l = L - u * UNIT_LINES, ea = u * DELTA_UNIT + s_lea[l];
            d = ((dmask[ea] & s_lma[l]) | (s_lmb[l] ? dmask[ea + 1] & s_lmb[l] : 0)) != 0;
        }
        const uint64_t m = __ballot(d);
        if (!m) continue;
        unsigned int base = 0;
        if (lane == 0) base = atomicAdd(nd, (unsigned int)__builtin_popcountll(m));
        base = __shfl(base, 0);
        if (d) list[base + __builtin_popcountll(m & ((1ull << lane) - 1))] = (uint16_t)L;
    }
}

// B2: the `nd` listed lines' stores: 16 bytes per lane, 8 lanes per line.  `tiles`: the group's tile ids, `out`: its first 16-byte chunk,
// `nq`: its chunks.
__device__ __forceinline__ void store_listed_lines(const uint16_t* list, int nd, const uint8_t* s_atlas, const uint8_t* tiles, u32x4* out, int nq,
                                                   int tid, int T) {
    for (int i = tid; i < nd * 8; i += T) {
        const int q = (int)list[i >> 3] * 8 + (i & 7);
        if (q >= nq) continue;                        // (past the end of an odd-sized last group: half a line)
        const int e = q / VEC_PER_ENV, k = q - e * VEC_PER_ENV;
        store_chunk16(s_atlas, tiles + e * CELLS, k, out + q);
    }
}

// ---- piece-granular stores (render_piece_bytes P < 128) --------------------------------------------------------------------------
// A P-byte piece (P divides 9408, so no piece crosses an env boundary and every env starts on the piece grid when the buffer does) is
// stored when a cell it is drawn from changed.  Stores are byte-masked and the memory side does not read a partial line back (FETCH_SIZE
// stays flat), but the store RATE falls with the piece: tools/ubench_sector_store.hip, 1 048 576 frames, a BossLevel-like dirty mix,
// ms against whole lines: 64 B 0.96, 32 B 1.81, 16 B 2.32 (WRITE_SIZE 0.87 / 0.74 / 0.74).  64-byte pieces ship: in the step loop they
// cut the headline's render by 3 % (profiles/render_pieces/); 32 and below lose more in rate than they save in bytes.
// Per env the cells of every piece come from a per-block table (s_pm: NP 49-bit masks), and ONE wave handles a dirty env: a lane per
// piece tests (dirty mask & piece cells), a ballot compacts the dirty pieces into the wave's own LDS list, and the wave stores them
// 16 bytes per lane, consecutive lanes on consecutive chunks.  The list is the wave's: no LDS atomic, no workgroup barrier.
__device__ __forceinline__ void wave_lds_sync() {     // the wave's own LDS writes are visible to its other lanes (no workgroup barrier)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int P>
__device__ __forceinline__ void init_piece_cells(uint64_t* s_pm, int tid, int nthreads) {
    for (int p = tid; p < Pieces<P>::NP; p += nthreads) s_pm[p] = line_cells(p * P, p * P + P);
}

// Stores the pieces of one env whose cells meet the dirty mask `m` (wave-uniform, nonzero).  Called by a whole wave; `wl` is the
// wave's list (NP entries), `t49` the env's 49 tile ids, `out` the env's first 16-byte chunk.
template <int P>
__device__ __forceinline__ void store_dirty_pieces(uint64_t m, const uint64_t* s_pm, uint16_t* wl, const uint8_t* s_atlas, const uint32_t* s_ct,
                                                   const uint8_t* t49, u32x4* out, int lane) {
    constexpr int NP = Pieces<P>::NP, S = Pieces<P>::S;
    int cnt = 0;
    for (int p0 = 0; p0 < NP; p0 += 64) {
        const int p = p0 + lane;
        const bool d = p < NP && (m & s_pm[p]) != 0;
        const uint64_t b = __ballot(d);
        if (d) wl[cnt + __builtin_popcountll(b & ((1ull << lane) - 1))] = (uint16_t)p;
        cnt += __builtin_popcountll(b);
    }
    wave_lds_sync();
    for (int i = lane; i < cnt * S; i += 64) {
        const int k = (int)wl[i / S] * S + (i & (S - 1));
        store_chunk16_t(s_atlas, s_ct, t49, k, out + k);
    }
    wave_lds_sync();                                  // the list is read before the wave's next env writes it
}

template <int G, int T, int SCHED, int P>
__global__ __launch_bounds__(T) void k_render_delta(int64_t n, const uint8_t* __restrict__ image, uint8_t* __restrict__ pixels,
                                                    uint8_t* __restrict__ shadow /* [n][49], row 0 = env 0 of this range */,
                                                    const uint8_t* __restrict__ atlas, const uint8_t* __restrict__ lut, int n_tiles) {
    static_assert(G % DELTA_UNIT == 0 && T % 64 == 0 && G % (T / 64) == 0, "whole units per group, whole envs per wave");
    constexpr int W = T / 64, EPW = G / W, GL = G / DELTA_UNIT * UNIT_LINES;
    __shared__ __attribute__((aligned(16))) uint8_t s_atlas[MAX_TILES * TILE_BYTES];
    __shared__ uint8_t s_lut[512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ngroups = (n + G - 1) / G;
    int64_t g, gend, gstep;
    if (SCHED == 0) { g = blockIdx.x; gend = ngroups; gstep = gridDim.x; }
    else { const int64_t per = (ngroups + gridDim.x - 1) / gridDim.x; g = blockIdx.x * per; gend = g + per < ngroups ? g + per : ngroups; gstep = 1; }
    // phase A's inputs of group `grp`, loaded ahead: 3 encoding bytes + the old id of this lane's cell in each of the wave's envs
    uint32_t o0[EPW], o1[EPW], o2[EPW], old[EPW];
    auto load = [&](int64_t grp) {
#pragma unroll
        for (int j = 0; j < EPW; ++j) {
            const int64_t env = grp * G + wave + j * W;
            o0[j] = o1[j] = o2[j] = old[j] = 0;
            if (grp < gend && lane < CELLS && env < n) {
                const uint8_t* o = image + env * OBS_BYTES + lane * 3;
                o0[j] = o[0]; o1[j] = o[1]; o2[j] = o[2];
                old[j] = shadow[env * CELLS + lane];
            }
        }
    };
    load_atlas_lds(s_atlas, atlas, n_tiles, threadIdx.x, T);
    load_lut_lds(s_lut, lut, threadIdx.x, T);
    if constexpr (P < LINE_BYTES) {
        // Pieces: the wave that finds an env's dirty mask (A) also stores its pieces, from the ids it has just written to LDS -- no
        // workgroup barrier in the loop, one tile buffer (a wave writes an env's ids again only after it has stored that env).
        __shared__ uint64_t s_pm[Pieces<P>::NP];
        __shared__ uint16_t s_wl[W][Pieces<P>::NP];
        __shared__ uint8_t s_tile1[G * CELLS + 8];
        __shared__ uint32_t s_ct[VEC_PER_ENV];
        init_piece_cells<P>(s_pm, threadIdx.x, T);
        init_chunk_table(s_ct, threadIdx.x, T);
        load(g);
        __syncthreads();                              // atlas, lut, piece and chunk tables loaded
        for (; g < gend; g += gstep) {
            const int64_t env0 = g * G;
            const int ne = (int)(n - env0 < G ? n - env0 : G);
            uint64_t dm[EPW];
#pragma unroll
            for (int j = 0; j < EPW; ++j) {
                const int e = wave + j * W;
                const bool live = lane < CELLS && e < ne;             // (delta_cell written out: shared, it costs this branch 1-4 VGPRs)
                const uint32_t id = live ? tile_id(s_lut, o0[j], o1[j], o2[j], lane) : 0;
                const bool d = live && id != old[j];
                dm[j] = __ballot(d);
                if (live) s_tile1[e * CELLS + lane] = (uint8_t)id;
                if (d) shadow[(env0 + e) * CELLS + lane] = (uint8_t)id;
            }
            load(g + gstep);                          // the next group's inputs ride under this group's stores
            wave_lds_sync();
#pragma unroll
            for (int j = 0; j < EPW; ++j) {
                const int e = wave + j * W;
                if (dm[j]) store_dirty_pieces<P>(dm[j], s_pm, s_wl[wave], s_atlas, s_ct, s_tile1 + e * CELLS, (u32x4*)(pixels + (env0 + e) * PIX_BYTES), lane);
            }
        }
        return;
    } else {
    __shared__ uint64_t s_lma[UNIT_LINES], s_lmb[UNIT_LINES];        // cells of the line's first / second env (0: one env)
    __shared__ uint8_t s_lea[UNIT_LINES];                              // the line's first env in the unit
    __shared__ uint64_t s_dmask[2][G];
    __shared__ uint8_t s_tile[2][G * CELLS + 8];
    __shared__ uint16_t s_list[2][GL];
    __shared__ unsigned int s_nd[2];
    init_line_table(s_lea, s_lma, s_lmb, threadIdx.x, T);
    load(g);
    __syncthreads();                                  // atlas, lut and line table loaded
    int buf = 0;
    for (; g < gend; g += gstep, buf ^= 1) {
        const int64_t env0 = g * G;
        const int ne = (int)(n - env0 < G ? n - env0 : G);
        // A: new ids, dirty masks, shadow write-back
#pragma unroll
        for (int j = 0; j < EPW; ++j) {
            const int e = wave + j * W;
            const uint64_t m = delta_cell(s_lut, o0[j], o1[j], o2[j], old[j], lane < CELLS && e < ne, lane, s_tile[buf] + e * CELLS, shadow + (env0 + e) * CELLS);
            if (lane == 0) s_dmask[buf][e] = m;
        }
        if (threadIdx.x == 0) s_nd[buf] = 0;
        __syncthreads();
        // B1: the group's dirty lines as a list
        const int nl = (int)(((int64_t)ne * PIX_BYTES + LINE_BYTES - 1) / LINE_BYTES);
        list_dirty_lines(s_dmask[buf], s_lea, s_lma, s_lmb, s_list[buf], &s_nd[buf], nl, threadIdx.x, T);
        __syncthreads();
        const int64_t gn = g + gstep;
        load(gn);                                     // the next group's inputs ride under this group's stores
        // B2: 16 bytes per lane, 8 lanes per listed line
        store_listed_lines(s_list[buf], (int)s_nd[buf], s_atlas, s_tile[buf], (u32x4*)(pixels + env0 * PIX_BYTES), ne * VEC_PER_ENV, threadIdx.x, T);
    }
    }
}

// k_render_dstore: the delta render of a step whose k_step has already found the dirty cells (step_dirty: the dirty masks in `dmask`, the
// new tile ids in the shadow).  Stores only: per G-env group it reads the G masks and the ids the stored lines are drawn from -- 8-byte
// pieces of the group's shadow rows, a piece loaded when a cell of it is drawn: its env is dirty, or the piece holds cells of the one line
// its env shares with the other env of its pair (envs 2k, 2k + 1 of a unit: line 73 + 147 k) and that line is stored; no encoding, no lut,
// no shadow write, no per-env phase.  Line list (B1) and stores (B2) as k_render_delta; the same static interleaved groups (SCHED 0).  The inputs are loaded a
// group ahead (the ids) and two groups ahead (the masks, which decide what ids are loaded), under the current group's stores.
constexpr int DSTORE_PIECES = 32 * CELLS / 8;                          // 8-byte shadow pieces of a 32-env group
template <int G, int T, int P>
__global__ __launch_bounds__(T) void k_render_dstore(int64_t n, uint8_t* __restrict__ pixels, const uint8_t* __restrict__ shadow /* [n][49], row 0 = env 0 of this range */,
                                                     const uint64_t* __restrict__ dmask /* [n] */, const uint8_t* __restrict__ atlas, int n_tiles) {
    static_assert(G == 32 && T >= DSTORE_PIECES && T >= G && T % 64 == 0, "one 8-byte shadow piece per thread and group");
    constexpr int GL = G / DELTA_UNIT * UNIT_LINES;
    __shared__ __attribute__((aligned(16))) uint8_t s_atlas[MAX_TILES * TILE_BYTES];
    __shared__ __attribute__((aligned(8))) uint8_t s_tile[2][G * CELLS + 8];
    load_atlas_lds(s_atlas, atlas, n_tiles, threadIdx.x, T);
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t ngroups = (n + G - 1) / G;
    const int64_t gstep = gridDim.x;
    int64_t g = blockIdx.x;
    // the dirty mask of env `tid` of group `grp` (0 past the end)
    auto load_mask = [&](int64_t grp) -> uint64_t {
        const int64_t env = grp * G + tid;
        return (tid < G && grp < ngroups && env < n) ? dmask[env] : 0ull;
    };
    // 8 ids of group `grp` from the shadow (bounds-checked at the end of the range)
    auto load_piece = [&](int64_t grp) -> uint2 {
        const int64_t base = grp * G * CELLS + 8 * tid, end = n * CELLS;
        if (base + 8 <= end) return *(const uint2*)(shadow + base);
        uint32_t w[2] = {0u, 0u};
        for (int i = 0; i < 8 && base + i < end; ++i) w[i >> 2] |= (uint32_t)shadow[base + i] << (8 * (i & 3));
        return make_uint2(w[0], w[1]);
    };
    if constexpr (P < LINE_BYTES) {
        // Pieces: only the dirty envs' ids are loaded (a piece of an env draws on that env's cells alone); one wave per dirty env stores
        // its pieces (store_dirty_pieces).  One workgroup barrier per group: the ids (two buffers) and the masks (three buffers: the
        // next group's masks are written while a slower wave may still read the current ones) are written in A and read behind it.
        constexpr int W = T / 64, EPW = G / W;
        __shared__ uint64_t s_pm[Pieces<P>::NP];
        __shared__ uint16_t s_wl[W][Pieces<P>::NP];
        __shared__ uint64_t s_dm3[3][G];
        __shared__ uint32_t s_ct[VEC_PER_ENV];
        const int wave = tid >> 6;
        init_piece_cells<P>(s_pm, tid, T);
        init_chunk_table(s_ct, tid, T);
        auto load_ids = [&](int64_t grp, int b) -> uint2 {
            if (tid >= DSTORE_PIECES || grp >= ngroups) return make_uint2(0u, 0u);
            const int ea = (8 * tid) / CELLS, eb = (8 * tid + 7) / CELLS;
            if (!s_dm3[b][ea] && !s_dm3[b][eb]) return make_uint2(0u, 0u);
            return load_piece(grp);
        };
        if (tid < G) s_dm3[0][tid] = load_mask(g);
        uint64_t mreg = load_mask(g + gstep);
        __syncthreads();                              // atlas, piece and chunk tables and the first group's masks
        uint2 idr = load_ids(g, 0);
        int buf = 0, mb = 0;
        for (; g < ngroups; g += gstep, buf ^= 1, mb = mb == 2 ? 0 : mb + 1) {
            const int64_t env0 = g * G;
            const int mn = mb == 2 ? 0 : mb + 1;
            if (tid < DSTORE_PIECES) *(uint2*)(s_tile[buf] + 8 * tid) = idr;
            if (tid < G) s_dm3[mn][tid] = mreg;
            __syncthreads();
            idr = load_ids(g + gstep, mn);            // the next group's ids and the masks of the one after it ride under the stores
            mreg = load_mask(g + 2 * gstep);
#pragma unroll
            for (int j = 0; j < EPW; ++j) {
                const int e = wave + j * W;
                const uint64_t m = s_dm3[mb][e];      // (0 past the end of the range)
                if (m) store_dirty_pieces<P>(m, s_pm, s_wl[wave], s_atlas, s_ct, s_tile[buf] + e * CELLS, (u32x4*)(pixels + (env0 + e) * PIX_BYTES), lane);
            }
        }
        return;
    } else {
    __shared__ uint64_t s_lma[UNIT_LINES], s_lmb[UNIT_LINES];
    __shared__ uint8_t s_lea[UNIT_LINES];
    __shared__ uint64_t s_dmask[2][G];
    __shared__ uint16_t s_list[2][GL];
    __shared__ unsigned int s_nd[2];
    init_line_table(s_lea, s_lma, s_lmb, tid, T);
    // the cells of the line an even env shares with the next one (its last 64 bytes), and of the odd env (its first 64)
    const uint64_t shared_a = line_cells(PIX_BYTES - LINE_BYTES / 2, PIX_BYTES), shared_b = line_cells(0, LINE_BYTES / 2);
    static_assert(PIX_BYTES % LINE_BYTES == LINE_BYTES / 2, "two envs of a pair share one line");
    // are the cells [c0, c1] of env e of the group drawn (masks: s_dmask[b]; envs past the end have none)
    auto drawn = [&](int b, int e, int c0, int c1) -> bool {
        if (s_dmask[b][e]) return true;
        const uint64_t pm = (c1 == 63 ? ~0ull : (2ull << c1) - 1) & ~((1ull << c0) - 1);
        const bool shared_stored = ((s_dmask[b][e & ~1] & shared_a) | (s_dmask[b][e | 1] & shared_b)) != 0;
        return shared_stored && (pm & ((e & 1) ? shared_b : shared_a)) != 0;
    };
    // this thread's 8-byte piece of group `grp`'s ids, if a cell of it is drawn
    auto load_ids = [&](int64_t grp, int b) -> uint2 {
        uint2 r = make_uint2(0u, 0u);
        if (tid >= DSTORE_PIECES || grp >= ngroups) return r;
        const int b0 = 8 * tid, b1 = b0 + 7, ea = b0 / CELLS, eb = b1 / CELLS;
        const bool need = eb == ea ? drawn(b, ea, b0 - ea * CELLS, b1 - ea * CELLS) : (drawn(b, ea, b0 - ea * CELLS, CELLS - 1) || drawn(b, eb, 0, b1 - eb * CELLS));
        if (!need) return r;
        return load_piece(grp);
    };
    if (tid < G) s_dmask[0][tid] = load_mask(g);
    uint64_t mreg = load_mask(g + gstep);
    __syncthreads();                                  // atlas, line table and the first group's masks
    uint2 idr = load_ids(g, 0);
    int buf = 0;
    for (; g < ngroups; g += gstep, buf ^= 1) {
        const int64_t env0 = g * G;
        const int ne = (int)(n - env0 < G ? n - env0 : G);
        // A: this group's ids and the next group's masks into LDS
        if (tid < DSTORE_PIECES) *(uint2*)(s_tile[buf] + 8 * tid) = idr;
        if (tid < G) s_dmask[buf ^ 1][tid] = mreg;
        if (tid == 0) s_nd[buf] = 0;
        __syncthreads();
        // B1: the group's dirty lines as a list (as k_render_delta)
        const int nl = (int)(((int64_t)ne * PIX_BYTES + LINE_BYTES - 1) / LINE_BYTES);
        for (int L0 = tid - lane; L0 < nl; L0 += T) {               // (list_dirty_lines written out: shared, it costs this kernel 3 SGPRs)
            const int L = L0 + lane;
            bool d = false;
            if (L < nl) {
                const int u = L / UNIT_LINES, l = L - u * UNIT_LINES, ea = u * DELTA_UNIT + s_lea[l];
                d = ((s_dmask[buf][ea] & s_lma[l]) | (s_lmb[l] ? s_dmask[buf][ea + 1] & s_lmb[l] : 0)) != 0;
            }
            const uint64_t m = __ballot(d);
            if (!m) continue;
            unsigned int base = 0;
            if (lane == 0) base = atomicAdd(&s_nd[buf], (unsigned int)__builtin_popcountll(m));
            base = __shfl(base, 0);
            if (d) s_list[buf][base + __builtin_popcountll(m & ((1ull << lane) - 1))] = (uint16_t)L;
        }
        // the next group's ids (its masks are in LDS since the barrier above) and the masks of the one after it ride under the stores
        idr = load_ids(g + gstep, buf ^ 1);
        mreg = load_mask(g + 2 * gstep);
        __syncthreads();
        // B2: 16 bytes per lane, 8 lanes per listed line (as k_render_delta)
        store_listed_lines(s_list[buf], (int)s_nd[buf], s_atlas, s_tile[buf], (u32x4*)(pixels + env0 * PIX_BYTES), ne * VEC_PER_ENV, tid, T);
    }
    }
}

// k_render_dstore_lw: k_render_dstore's piece branch as a queue.  Eight waves only store and a ninth, the loader, only loads; a group's
// dirty envs go to the storing waves as they come free; groups go to blocks from one ticket counter, and ONE block runs per CU.
//   * the loader (wave 8) issues every global load of the loop -- the 196 eight-byte shadow pieces of the NEXT group's dirty envs (four
//     rounds of 64 lanes) and the 32 masks of the group after it -- waits for them and writes them to LDS inside its own branch: nothing
//     it loads is in a register where the two paths join, and the storing waves' path holds no vmcnt wait (k_render_dstore's waves
//     carry ids and masks in registers across their stores and drain their store queue once per group; measured, the drain costs
//     nothing -- profiles/render_store_queue/README.md -- the loader is here for what follows);
//   * one workgroup barrier per group, reached by all nine waves after `if (loader) ... else ...`; ids in two buffers, masks (and what
//     goes with them: the list of dirty envs, its length and take counter, the group's index) in three -- a buffer the loader writes
//     between barriers k and k + 1 was last read between barriers k - 1 and k;
//   * the loader lists the group's dirty envs (a ballot over the 32 masks); a storing wave takes its next env with one LDS atomic add
//     by one lane, so the group's bytes spread over the waves as they come free (statically, wave w stores envs w, w + 8, w + 16,
//     w + 24: 60 % of env-steps are clean and the slowest wave of a group carries about twice the mean);
//   * groups come from ONE ticket counter, two consecutive groups per ticket (16 384 tickets per launch at 1 048 576 envs), in order:
//     the chip's stores advance through the buffer as one compact window, as k_render_q's do -- with the static interleaved split a
//     block runs as far ahead as its own groups let it.  The loader takes a ticket one ahead of the one it prefetches for (the spare
//     rides in LDS, not in a register) and publishes every phase's group in LDS; all nine waves read "no more groups" from there
//     behind the barrier and so run the same number of barriers.  Counters: words of the handle's render_tickets that k_render_q
//     leaves alone; the last block to leave zeroes them, as there (its comment: two launches never share them; every ticket a block
//     took has returned -- it went through LDS -- before the block departs).
// The stored bytes are k_render_dstore's: the same masks select the same pieces (store_dirty_pieces).
constexpr int DSTORE_LW_T = 9 * 64;                                    // 8 storing waves + the loader
constexpr int DSTORE_LW_K = 2;                                         // groups per ticket
constexpr int DSTORE_LW_COUNTER = 32 * 64, DSTORE_LW_DEPARTED = 33 * 64;     // words of render_tickets (k_render_q: rows 0 .. 8)
__device__ __forceinline__ int64_t uniform64(int64_t v) {        // a wave-uniform value read from LDS, for the scalar unit
    return (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)((uint64_t)v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)v));
}
template <int P>
__global__ __launch_bounds__(DSTORE_LW_T) void k_render_dstore_lw(int64_t n, uint8_t* __restrict__ pixels, const uint8_t* __restrict__ shadow /* [n][49], row 0 = env 0 of this range */,
                                                                  const uint64_t* __restrict__ dmask /* [n] */, const uint8_t* __restrict__ atlas, int n_tiles,
                                                                  unsigned int* __restrict__ tickets) {
    static_assert(P < LINE_BYTES, "pieces");
    constexpr int G = 32, T = DSTORE_LW_T, W = 8, K = DSTORE_LW_K, ROUNDS = (DSTORE_PIECES + 63) / 64;
    __shared__ __attribute__((aligned(16))) uint8_t s_atlas[MAX_TILES * TILE_BYTES];
    __shared__ __attribute__((aligned(8))) uint8_t s_tile[2][G * CELLS + 8];
    __shared__ uint64_t s_pm[Pieces<P>::NP];
    __shared__ uint16_t s_wl[W][Pieces<P>::NP];
    __shared__ uint64_t s_dm3[3][G];
    __shared__ uint32_t s_ct[VEC_PER_ENV];
    __shared__ uint8_t s_list[3][G];                  // the group's dirty envs, ...
    __shared__ unsigned int s_cnt[3], s_next[3];      // ... how many, and how many the storing waves have taken
    __shared__ int64_t s_grp[3];                      // the group of the phase (>= ngroups: none, and none behind it)
    __shared__ unsigned int s_spare;                  // the ticket taken ahead
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool loader = wave == W;
    const int64_t ngroups = (n + G - 1) / G;
    load_atlas_lds(s_atlas, atlas, n_tiles, tid, T);
    init_piece_cells<P>(s_pm, tid, T);
    init_chunk_table(s_ct, tid, T);
    // One step of the loader, "iteration k" (k = -2, -1: the prologue): the ids of phase k + 1 (group g1, masks in buffer m1) into tile
    // buffer tb and the masks of phase k + 2 into buffer m2, with the list, the counters and the group's index.  Every load is issued
    // without a branch around it (a lane with nothing to load reads the range's first bytes), so that they are in flight together.
    unsigned int* counter = tickets + DSTORE_LW_COUNTER;
    int64_t g1 = ngroups;                             // (no phase -1)
    auto loader_step = [&](int k, int m1, int tb, int m2) {
        const int64_t end = n * CELLS;
        const bool opens = (k + 2) % K == 0;          // every K-th phase opens a ticket: the spare one from LDS, the next spare into it below
        int64_t g2 = g1 + 1;
        unsigned int spare = 0;
        if (opens) {
            g2 = (int64_t)s_spare * K;
            if (lane == 0) spare = atomicAdd(counter, 1u);
        }
        uint2 v[ROUNDS];
        bool need[ROUNDS], tail = false;
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int p = r * 64 + lane, pc = p < DSTORE_PIECES ? p : DSTORE_PIECES - 1;
            const int64_t base = g1 * G * CELLS + 8 * p;
            // an 8-byte piece is loaded when an env it holds cells of is dirty (masks past the end of the range are 0)
            need[r] = p < DSTORE_PIECES && g1 < ngroups && (s_dm3[m1][(8 * pc) / CELLS] || s_dm3[m1][(8 * pc + 7) / CELLS]);
            const bool whole = base + 8 <= end;
            tail |= need[r] && !whole;
            v[r] = *(const uint2*)(shadow + (need[r] && whole ? base : 0));
        }
        const int64_t env = g2 * G + lane;
        const bool live = lane < G && g2 < ngroups && env < n;
        uint64_t m = dmask[live ? env : 0];
        if (!live) m = 0;
        if (__any(tail)) {                            // the range's ids end inside a piece: byte by byte (as k_render_dstore's load_piece)
#pragma unroll
            for (int r = 0; r < ROUNDS; ++r) {
                const int64_t base = g1 * G * CELLS + 8 * (r * 64 + lane);
                if (!need[r] || base + 8 <= end) continue;
                uint32_t w[2] = {0u, 0u};
                for (int i = 0; i < 8 && base + i < end; ++i) w[i >> 2] |= (uint32_t)shadow[base + i] << (8 * (i & 3));
                v[r] = make_uint2(w[0], w[1]);
            }
        }
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int p = r * 64 + lane;
            if (p < DSTORE_PIECES) *(uint2*)(s_tile[tb] + 8 * p) = need[r] ? v[r] : make_uint2(0u, 0u);
        }
        if (lane < G) s_dm3[m2][lane] = m;
        const uint64_t dirty = __ballot(m != 0);
        if (m) s_list[m2][__builtin_popcountll(dirty & ((1ull << lane) - 1))] = (uint8_t)lane;
        if (lane == 0) {
            s_cnt[m2] = (unsigned int)__builtin_popcountll(dirty);
            s_next[m2] = 0;
            s_grp[m2] = g2;
            if (opens) s_spare = spare;
        }
        g1 = g2;
    };
    if (loader) {
        if (lane == 0) s_spare = atomicAdd(counter, 1u);
        wave_lds_sync();
        loader_step(-2, 2, 1, 0);                     // phase 0's masks
        wave_lds_sync();
        loader_step(-1, 0, 0, 1);                     // phase 0's ids, phase 1's masks
    }
    __syncthreads();                                  // atlas, piece and chunk tables; phase 0's ids and masks, phase 1's masks
    int buf = 0, mb = 0;
    for (int k = 0;; ++k, buf ^= 1, mb = mb == 2 ? 0 : mb + 1) {
        const int64_t g = uniform64(s_grp[mb]);
        if (g >= ngroups) break;
        if (loader) {
            const int m1 = mb == 2 ? 0 : mb + 1, m2 = m1 == 2 ? 0 : m1 + 1;
            loader_step(k, m1, buf ^ 1, m2);
        } else {
            const int64_t env0 = g * G;
            const unsigned int cnt = __builtin_amdgcn_readfirstlane(s_cnt[mb]);
            for (;;) {
                unsigned int i = 0;
                if (lane == 0) i = atomicAdd(&s_next[mb], 1u);
                i = __builtin_amdgcn_readfirstlane(i);
                if (i >= cnt) break;
                const int e = __builtin_amdgcn_readfirstlane(s_list[mb][i]);
                store_dirty_pieces<P>(s_dm3[mb][e], s_pm, s_wl[wave], s_atlas, s_ct, s_tile[buf] + e * CELLS, (u32x4*)(pixels + (env0 + e) * PIX_BYTES), lane);
            }
        }
        __syncthreads();
    }
    if (tid == W * 64) {
        unsigned int* departed = tickets + DSTORE_LW_DEPARTED;
        if (atomicAdd(departed, 1u) == gridDim.x - 1) { atomicExch(counter, 0u); atomicExch(departed, 0u); }
    }
}
#endif  // __HIPCC__
