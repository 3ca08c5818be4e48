// bbai_reseedk.hpp -- env.seed(s); env.reset() for LISTED envs of a live batch, on the device (bbai_reseed, bbai_engine.hip).
//   k_reseed_seed     lane = list entry: the env's MT19937 stream restarts from its seed (seed_env, as k_seed), its hot state and every hot slot of
//                     its ring become the empty state of k_init_hot (so the generator's locked_room chain starts at None), its byte in the
//                     CURRENT window's buffer is cleared (what it consumed there needs no refill any more: its whole ring is regenerated), and it
//                     is put on a work list and into a `pending` / `first_slot` plane that only reseeds use: D levels (D - 1 in place) from slot 0.
//   (generation)      k_pregen / k_pregen_lane, unchanged, `listed` over that list and that plane.
//   k_reseed_consume  wave = list entry: consume_env (bbai_stepk.hpp) on slot 0 under the current window's bookkeeping -- the copy (or, in place,
//                     the move) into the live state, the verifier view, planes, first observation -- plus the reset total and an expert plan that
//                     no longer matches any step.
// A SHORT reseed (option "reseed_levels" = k, 0 < k < D - inplace) books k levels instead of the ring (bbai_reseed hands k_reseed_seed the
// slots that get NO level: D - k instead of `inplace` -- the kernel and its signature are the whole-ring reseed's): the generator fills slots 0 .. k - 1 and
// slot k keeps the empty frozen Hot written here, so the env's ordinary move into slot k (consume_env, advance_load / advance_finish) PARKS it;
// no step kernel knows.  That move reads slot k's RECORD too (Prog, start_carry -> pos[], window plane, C plane row, first observation), and
// nothing wrote one for this seed.  It is safe because every slot an env can move into holds a record some generator run completed:
//   * bbai_seed fills slots 0 .. D - 1 - inplace of every env, and k <= D - 1 - inplace, so slot k is one of them (the in-place layout's empty
//     slot D - 1, zeros since bbai_create, is never a parking slot; bbai_reset calls can walk a parked env there, 2B consume-ticks behind the
//     reseed at the earliest, and k_gate has by then waited for the refill that the reseed's own consume booked for slot D - 1);
//   * later writers of a slot are the generators alone (whole records, each behind the last on the look-ahead streams) and, in place, the
//     steps of the episode that lived there -- which change cells and id bytes but never Prog, and leave pos[] of a carried object where it
//     was (apply_start_carry, bbai_step.hpp): start_carry and the position it indexes stay what a generator wrote, inside the env's rows.
// What the parked env shows is that old level's first observation under the empty pose: unspecified by contract, never stepped (frozen).
// An env listed twice (a caller error) is seeded and consumed ONCE: k_reseed_seed claims an env by its bit of `claim` and skips an entry
// whose env is taken, k_reseed_consume gives the bit back and skips an entry whose env's bit is gone.  So the work list holds every env at
// most once (its sub-lists cannot overflow: k_compact's bound), and `claim` is all zero between calls.
// Grids follow the list's length, never the batch's.  No LDS, no scratch.
// Part of bbai_engine.hip's translation unit: included behind bbai_statek.hpp.  Both kernels are templates (one instantiation each, <0>) that
// bbai_reseed, at the end of bbai_engine.hip, launches first: their code lies behind every earlier kernel's (bbai_statek.hpp says why).
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include "bbai_types.hpp"
#include "bbai_kernels.hpp"
#include "bbai_seed.hpp"
#include "bbai_step.hpp"
#include "bbai_stepk.hpp"
#include "bbai_bot.hpp"

using namespace bbai;

template <int TAIL = 0>
__global__ __launch_bounds__(64) void k_reseed_seed(int64_t n, const int64_t* __restrict__ ids /* or NULL: env k */, const uint64_t* __restrict__ seeds, int64_t count,
                                                    uint32_t* __restrict__ mts, int32_t* __restrict__ mtis, uint8_t* __restrict__ mtpar /* or NULL */,
                                                    Hot* __restrict__ hots, Hot* __restrict__ next_hots, int depth, int spare /* slots of the ring that get no level: `inplace` (the whole ring), D - k (a short reseed) */,
                                                    uint8_t* __restrict__ cur_pending /* the current window's buffer */,
                                                    uint8_t* __restrict__ rs_pending, uint8_t* __restrict__ rs_first, uint32_t* __restrict__ claim,
                                                    int32_t* __restrict__ rs_list, uint32_t* __restrict__ rs_count) {
    const int64_t cap = gen_sublist_cap(n);
    for (int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x; k < count; k += (int64_t)gridDim.x * 64) {
        const int64_t env = ids ? ids[k] : k;
        if (env < 0 || env >= n) continue;
        const uint32_t bit = 1u << (env & 31);
        if (atomicOr(&claim[env >> 5], bit) & bit) continue;          // listed twice: the first entry has it
        seed_env(seeds[k], mts + env * MT_N);
        mtis[env] = MT_N;                                             // (k_seed: the first draw twists)
        if (mtpar) mtpar[env] = 0;
        Hot h;                                                        // k_init_hot's empty state: slot 0 (in place: the live slot is the empty slot D - 1), frozen
        memset(&h, 0, sizeof(h));
        h.carry = NONE8; h.frozen = 1; h.last_locked = NONE8;
        h.pre4 = 0xFFFFFFFFu;
        hots[env] = h;
        for (int d = 0; d < depth; ++d) next_hots[ring_at(d, env, depth)] = h;
        cur_pending[env] = 0;
        rs_pending[env] = (uint8_t)(depth - spare);                   // slots 0 .. depth - spare - 1 get the new stream's first levels; the next slot of a short reseed parks the env
        rs_first[env] = 0;
        const int j = (int)((env >> 6) % SHARDS);                     // k_compact's sub-list of the env's 64-env block: at most `cap` different envs
        const uint32_t at = atomicAdd(&rs_count[j * GEN_COUNT_U32], 1u);
        if ((int64_t)at < cap) rs_list[(int64_t)j * cap + at] = (int32_t)env;
    }
}

template <int TAIL = 0>
__global__ __launch_bounds__(256) void k_reseed_consume(LevelCfg c, int64_t n, const int64_t* __restrict__ ids /* or NULL: env k */, int64_t count,
                                                        uint32_t* __restrict__ claim, uint8_t* recs, Hot* __restrict__ hots, uint64_t* __restrict__ stales,
                                                        uint8_t* next_recs, const Hot* __restrict__ next_hots, uint32_t* __restrict__ vheads,
                                                        uint64_t* __restrict__ vsets, unsigned long long* __restrict__ totals, int depth,
                                                        uint8_t* __restrict__ pending, uint8_t* __restrict__ first_slot, uint32_t* __restrict__ win_meta,
                                                        uint8_t* __restrict__ image, uint8_t* __restrict__ dirs, uint8_t* __restrict__ vplane /* or NULL */,
                                                        uint16_t* __restrict__ fcache, uint8_t* __restrict__ lsm_arr /* or NULL */, int inplace,
                                                        uint8_t* __restrict__ cplane /* or NULL */, uint8_t* __restrict__ bot_states /* or NULL */, int bot_stack) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t k = wave; k < count; k += nwaves) {
        const int64_t env = ids ? ids[k] : k;
        if (env < 0 || env >= n) continue;
        const uint32_t bit = 1u << (env & 31);
        uint32_t old = 0;
        if (lane == 0) old = atomicAnd(&claim[env >> 5], ~bit);
        if (!(__shfl(old, 0) & bit)) continue;                        // (the env's other entry was here)
        consume_env(c, n, env, 0, lane, recs, hots, stales, next_recs, next_hots, vheads, vsets, depth, pending, first_slot, win_meta,
                    image + env * OBS_BYTES, dirs, vplane, fcache, lsm_arr, inplace != 0, cplane);
        if (lane == 0) {
            count_resets(totals, 1u, (unsigned int)(env >> 6));
            if (bot_states) ((BotState*)(bot_states + env * (int64_t)bot_state_bytes(bot_stack)))->next_step = 0;      // (k_state_load: the next decision starts a fresh plan)
        }
    }
}
