// bbai_kernels.hpp -- what the engine's translation units and kernel headers share on the device side: the 16-byte vector type, the view's
// cell count, the windows' bookkeeping and its constants, the look-ahead ring's addressing and the live record of both state layouts, the
// refill list's shape, the listed-env observation kernels' argument record (EnvList) and item skeleton (list_item_*), the lane-group
// context of the generators.  A definition that one kernel family alone uses is in that family's header.
// (bbai_engine.hip: the host side; it includes a header per kernel family -- bbai_stepk.hpp, bbai_pregen.hpp, bbai_ring.hpp, bbai_botk.hpp,
// bbai_render.hpp, bbai_gridk.hpp, bbai_tokens.hpp, bbai_demo.hpp, bbai_statek.hpp, bbai_reseedk.hpp -- and each of them includes this one.  bbai_genlane.hip: k_pregen_lane.)
#pragma once
#include <hip/hip_runtime.h>
#include "bbai_types.hpp"

namespace bbai {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int CELLS = VIEW * VIEW;
constexpr int AGENT_CELL = 3 * VIEW + 6;                        // the agent's own cell of the view: (3, 6) (tile_id in bbai_render.hpp, step_dirty in bbai_stepk.hpp)
static_assert(AGENT_CELL == 3 * VIEW + 6, "the agent stands in the middle of the view's last row");

// ---- the windows' bookkeeping: no lists, no same-address atomics on the step path -----------------------------------------------
// Rounds 1-4 compacted the finished envs of every tick into a window list for the refill (one RETURNING atomic per stepping wave
// on ONE address: ~2 700 of them per step at 262 144 reset-heavy envs, served at ~11 ns each -- half of that k_step's time) and made
// the step stream wait, at the start of window w + 2, for the refill of window w (an env MIGHT finish on every tick).  Now:
//   * what a stepping wave leaves behind is one fire-and-forget add to a sharded total (SHARDS cache lines) and per-env bytes; the
//     refill's work list is built where it costs nothing: k_compact, on the look-ahead stream in front of k_pregen, turns the window's
//     `pending` bytes (n bytes per B ticks) into SHARDS dense sub-lists (one returning atomic per 64 envs that hold a finished one,
//     spread over SHARDS counters), which k_pregen walks as ONE list through a prefix of the sub-counts -- the same perfectly
//     balanced entry-per-group distribution as before.  (Letting the generator's groups scan the bytes themselves was measured
//     first -- lease r05a: a group then finds 0 to 4 envs where its neighbour finds one, a wave lives as long as its unluckiest
//     group, and the mazes' steps slowed by 10-30 % under the generator's idle lanes.)
//   * every window records M = the most often ONE env finished in it (1 unless short episodes repeat inside a window: the
//     rare atomicMax in the consume paths); an env's unrefilled slots are <= the sum of M over the windows whose refill has not
//     landed, so window x may start as soon as that sum is <= B (every env then still has B ready levels, and a window consumes
//     at most B) -- k_gate, one wave on the step stream at every window start, waits for exactly that instead of for "refill
//     w - 2 has landed".  A reset storm (a million maze envs timing out on the same tick: 37 ms of generator time) then runs
//     UNDER the following windows instead of stopping the step stream, as long as no env finishes B more times meanwhile.
//   * NWIN = 34 window buffers (pending / first_slot / meta): up to 33 refills can be outstanding (B + 1 of them for B <= 32).
//   * bbai_reseed (bbai_reseedk.hpp) is no consume-tick, but it books the listed env's reset into the CURRENT window like any finished
//     env's: after clearing the env's byte there (its whole ring is regenerated: what it consumed before needs no refill), pending 1,
//     first slot 0.  One env can so consume B + 1 slots in one window (a reseed in front of the window's first tick, then a finish on
//     every tick).  M records that truthfully through the same atomicMax, the sum over the open windows then exceeds B while this
//     window is among them, and k_gate simply holds the next window until THIS window's refill has landed; the env's ring was full at
//     the reseed, so the B + 1 <= 2B levels are there.  The call waits for every refill launched before it, so no other window holds a
//     byte of a listed env.
// tests/test_ring_protocol.py models the rule (sufficient, and the ring depths stay tight); tests/test_ring_protocol_reseed.py adds the reseed.
constexpr int NWIN = 34;                // window buffers (above): at most 33 refills outstanding, whatever B
constexpr int META_U32 = 32;            // uint32 per window buffer's meta line: [0] = M when > 1 (atomicMax)
constexpr int SHARDS = 64;              // cache lines the reset total is spread over (k_step: shard = block & 63)
constexpr int SHARD_U64 = 16;           // uint64 per shard: one 128-byte line each
enum : int { FLOW_REFILLED = 0 /* windows whose refill has landed */, FLOW_GATE_TIMEOUTS = 1, FLOW_PROBE = 2 /* probe_stream's flag */, FLOW_GEN_FAILURES = 3 /* levels the generator gave up on */, FLOW_WORDS = 16 };
constexpr int GEN_COUNT_U32 = 32;       // uint32 per sub-list counter of the refill list: one 128-byte line each
__host__ __device__ __forceinline__ int64_t gen_sublist_cap(int64_t n) { return ((n + 63) / 64 + SHARDS - 1) / SHARDS * 64; }      // entries a sub-list can get: its waves x 64

// The look-ahead ring is ENV-MAJOR: entry (slot, env) of next_rec / next_hot / next_obs is number env * depth + slot -- an env's D levels
// lie together.  (Slot-major, rounds 1-4a, put the 64 envs of a stepping wave into up to 64 regions n * rec_bytes apart as soon as
// the live records are ring slots: profiles/r04/inplace_ring_depth_ab.jsonl, k_step 0.029 -> 0.035 ms from D = 5 to D = 65.)
__device__ __forceinline__ int64_t ring_at(int slot, int64_t env, int depth) { return env * depth + slot; }

// ---- the in-place layout (bbai_env::inplace, chosen at bbai_create) ------------------------------------------------------------
// Classic layout: every env has a live record of its own (rec[env]); a finished env's next level is COPIED out of its look-ahead
// slot (1.3 - 1.7 KB + the window plane), by a k_consume launch behind every step or by the stepping wave.  On reset-heavy small
// shards (single rooms: 2 % of the envs finish on every step) that second dependent launch is 40 % of a step (profiles/r04/NOTES.md
// section 2), and doing its work inside the stepping waves costs more than the launch.  In-place layout: the live record of an env
// IS the ring slot its episode was generated into -- the slot BEFORE hot.slot -- and a finished env just moves on to the next
// slot: nothing is copied, the stepping LANE loads the new pose and program (one round trip), emits the first observation with the
// step's own window pipeline and swaps the SoA state.  The ring is one slot deeper (2B + 1: the live one + the 2B look-ahead
// levels of the classic ring); the slot an episode leaves is the one the window's refill regenerates.  rec[] stays allocated as the
// staging area of export / import / checkpoints.  No window plane in this layout (the window comes out of the record's appearance
// plane: measures equal on the shards this is for).
__device__ __forceinline__ int live_slot(int next_slot, int depth) { return (next_slot ? next_slot : depth) - 1; }
__device__ __forceinline__ uint8_t* live_rec(const LevelCfg& c, int64_t n, int64_t env, uint8_t* recs, uint8_t* ring, int depth, int next_slot) {
    (void)n;
    return ring ? ring + ring_at(live_slot(next_slot, depth), env, depth) * (int64_t)c.rec_bytes : recs + env * (int64_t)c.rec_bytes;
}

// ---- observations of LISTED envs, drawn from the live state (bbai_gridk.hpp: k_render_grid, k_full_obs; bbai_viewn.hpp: k_view_obs) -------
// The batch's live state, the listed envs, and where their frames go: frame k of `out` is the observation of env ids[k].  Each family's
// argument struct opens with this record (bbai_engine.hip: env_list fills it).
struct EnvList {
    LevelCfg c;
    int64_t n;
    const uint8_t* recs;
    const uint8_t* ring;         // in-place layout: the live records are ring slots; else NULL
    int depth;
    const Hot* hots;
    const int64_t* ids;          // NULL: envs 0 .. count - 1
    int64_t count;
    uint8_t* out;
};

// (env, Hot) of entry k: the Hot as one 16-byte load; env = -1 and a zero Hot for an id outside [0, n)
__device__ __forceinline__ void list_entry(const EnvList& l, int64_t k, int64_t& env, u32x4& h) {
    env = l.ids ? l.ids[k] : k;
    h = u32x4{0u, 0u, 0u, 0u};
    if (env >= 0 && env < l.n) h = ((const u32x4*)l.hots)[env];
    else env = -1;
}
// the live record of entry (env, h) in both state layouts (h.w >> 24 = Hot::slot), NULL for env = -1
__device__ __forceinline__ const uint8_t* list_rec(const EnvList& l, int64_t env, const u32x4& h) {
    return env >= 0 ? live_rec(l.c, l.n, env, (uint8_t*)l.recs, (uint8_t*)l.ring, l.depth, l.ring ? (int)(h.w >> 24) : 0) : nullptr;
}

// The item skeleton of the persistent blocks of k_full_obs and k_view_obs<V>, in pieces: an item is `epi` consecutive entries, one lane
// each; block b works items b, b + gridDim.x, ...  The kernel keeps (env, h) of its CURRENT item in registers: list_item_load ahead of
// the loop for the first item and, under an item's work, for the next one; behind a barrier list_item_park puts them, with the record,
// where the whole block reads them; the item's frames, built in LDS, leave through list_item_store.  The barriers are the kernel's.
__device__ __forceinline__ int list_item_envs(const EnvList& l, int64_t first, int epi) { return (int)(l.count - first < epi ? l.count - first : epi); }
// lane tid's entry of item `item`: returns its env, the Hot in h (-1, h as it was: the item has no such entry).  Whether there IS such an
// item is the block's question, not the lane's: the kernel asks it at the call
__device__ __forceinline__ int64_t list_item_load(const EnvList& l, int64_t item, int epi, int tid, u32x4& h) {
    int64_t env = -1;
    if (tid < epi && item * epi + tid < l.count) list_entry(l, item * epi + tid, env, h);
    return env;
}
// lane tid (< the item's envs) parks its entry and its live record in LDS
__device__ __forceinline__ void list_item_park(const EnvList& l, int tid, int64_t env, const u32x4& h, Hot* s_hot, const uint8_t** s_rec) {
    ((u32x4*)s_hot)[tid] = h;
    s_rec[tid] = list_rec(l, env, h);
}
// `bytes` bytes of frames from LDS to dst (16-byte aligned) as 16-byte nontemporal chunks, the tail -- the last item's only -- byte by byte
template <int BLOCK>
__device__ __forceinline__ void list_item_store(uint8_t* dst, const uint8_t* s_frames, int bytes, int tid) {
    const int chunks = bytes >> 4;
    for (int q = tid; q < chunks; q += BLOCK) __builtin_nontemporal_store(((const u32x4*)s_frames)[q], (u32x4*)dst + q);
    for (int b = (chunks << 4) + tid; b < bytes; b += BLOCK) dst[b] = s_frames[b];
}

// One env per group of G lanes, 64 / G envs per wavefront (bbai_gen.hpp "Execution model").  sync() orders the group's LDS
// accesses: it is reached under divergent control flow (the groups of a wave are in different places of the generator),
// so it is a wave-local fence, never a workgroup barrier -- the workgroup is one wave.
template <int G>
struct GroupCtx {
    static constexpr int kLanes = G;
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x & (G - 1); }
    __device__ __forceinline__ int nlanes() const { return G; }
    __device__ __forceinline__ void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    __device__ __forceinline__ uint32_t shfl(uint32_t v, int src) const { return __shfl(v, src, G); }
    __device__ __forceinline__ uint32_t shfl_up1(uint32_t v) const { uint32_t t = __shfl_up(v, 1, G); return lane() == 0 ? 0u : t; }
    __device__ __forceinline__ uint32_t shfl_down1(uint32_t v) const { uint32_t t = __shfl_down(v, 1, G); return lane() == G - 1 ? 0u : t; }
    __device__ __forceinline__ unsigned long long ballot(bool p) const {     // the group's share of the wave's ballot: bit k = lane k of the group
        const unsigned long long b = __ballot(p);
        constexpr unsigned long long m = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
        return (b >> ((int)threadIdx.x & ~(G - 1) & 63)) & m;
    }
    __device__ __forceinline__ bool any(bool p) const {
        const unsigned long long b = __ballot(p);
        constexpr unsigned long long m = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
        return ((b >> ((int)threadIdx.x & ~(G - 1) & 63)) & m) != 0ull;
    }
};

// k_pregen_lane's launch arguments: filled by bbai_engine.hip (launch_pregen_lane), launched by bbai_genlane.hip (bbai_lane_launch)
struct LaneLaunch {
    LevelCfg cfg; int64_t n; uint8_t* next_rec; Hot* next_hot; uint32_t* mt; uint32_t* mtt; uint8_t* mtpar; int32_t* mti;
    const int32_t* gen_list; const uint32_t* gen_count; int depth; uint8_t* pending; const uint8_t* first_slot;
    unsigned long long* fails; uint8_t* next_obs; const uint8_t* tmpl; int lane_words; unsigned blocks; hipStream_t stream;
};
void bbai_lane_launch(const LaneLaunch& a);

}  // namespace bbai
