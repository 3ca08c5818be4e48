// bbai_botk.hpp -- the expert's kernels.
//   k_bot<W>       lane = env: one decision of the reference's GOFAI expert (babyai/bot.py) per env, W = occupancy target
//                  (bbai_bot.hpp); only launched by bbai_bot_act / bbai_bot_rollout.
//   k_botg<G, W>   experiment builds only (BBAI_BOT_GROUP_BUILD=1): one lane group per env.
// Part of bbai_engine.hip's translation unit: included where the code stood, at global scope.  The launches are bbai_engine.hip's (bot_launch).
#pragma once
#include <hip/hip_runtime.h>
#include "bbai_types.hpp"
#include "bbai_kernels.hpp"
#include "bbai_bot.hpp"

using namespace bbai;

// The reference's expert for every env (babyai/bot.py Bot.replan): lane = env, grid-stride over the batch with one BFS
// scratch block per resident thread.  A new episode (step_count == 0) starts a fresh Bot.
template <int WAVES_PER_SIMD>
__global__ __launch_bounds__(64, WAVES_PER_SIMD) void k_bot(LevelCfg c, int64_t n, const uint8_t* __restrict__ recs, const uint8_t* __restrict__ ring /* in-place layout: the live records are ring slots; else NULL */,
                                            int depth, const Hot* __restrict__ hots,
                                            const uint64_t* __restrict__ stales, uint8_t* __restrict__ states, int stack_cap,
                                            uint16_t* __restrict__ works, uint32_t* __restrict__ slow_rows, int eager, const uint8_t* __restrict__ prev_actions,
                                            uint8_t* __restrict__ out, unsigned long long* __restrict__ stats,
                                            int dead_action /* what a bot that gave up emits: BOT_DEAD, or A_RESET_ENV in a rollout */,
                                            uint8_t* __restrict__ gave_up /* or NULL: [n] 1 where the bot gave up at this decision */) {
    // the searches' hot row masks (expandable / queued / seen), [row][lane] in LDS: every lane on its own bank
    extern __shared__ uint32_t s_rows[];              // [R_FAST][H][64] row masks, then the queue ring uint16 [BOT_RING][64]
    uint16_t* s_ring = (uint16_t*)(s_rows + R_FAST * c.H * 64);
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
    BotWork w;
    w.eager = eager;
    w.ring = s_ring + threadIdx.x; w.ring_stride = 64; w.ring_size = BOT_RING;
    w.rows_fast = s_rows + threadIdx.x; w.rstride_fast = 64; w.rows_h = c.H;
    w.rows_slow = slow_rows + tid * ((R_ALL - R_FAST) * MAX_W); w.rstride_slow = 1;
    // per-thread contiguous scratch: measured faster than lane-interleaving it (BossLevel 262144 envs 12.8 vs 17.6 ms per
    // decision batch) -- the lanes' searches diverge at once, so an interleaved line holds one useful 2-byte element
    w.cells = c.W * c.H;                                    // 64 cells (512 B of scratch) for an 8x8 room, 484 for a 3x3 maze
    w.base = works + tid * (int64_t)(4 * w.cells);
    w.stride = 1;
    for (int64_t i = tid; i < n; i += nthreads) {
        const Hot h = hots[i];
        if (h.frozen) { out[i] = A_DONE; if (gave_up) gave_up[i] = 0; continue; }
        BotState& st = *(BotState*)(states + i * (int64_t)bot_state_bytes(stack_cap));
        const bool first = h.step == 0 || st.next_step != h.step;       // (bot_decide applies the same rule)
        const int taken = (prev_actions && !first) ? prev_actions[i] : -1;
        const bool was_dead = !first && st.dead;
        const int a = bot_decide(c, live_rec(c, n, i, (uint8_t*)recs, (uint8_t*)ring, depth, h.slot), h, stales[i], st, stack_cap, w, first, taken);
        out[i] = (uint8_t)(a == BOT_DEAD ? dead_action : a);
        if (gave_up) gave_up[i] = a == BOT_DEAD ? 1 : 0;
        if (a == BOT_DEAD && !was_dead) atomicAdd(&stats[st.dead == DEAD_CAPACITY ? 1 : 0], 1ull);
    }
}

// BBAI_BOT_GROUP_BUILD=1 (experiment builds only; the shipped library has no k_botg): the expert as one 16-lane group per env.  Built, verified on
// the host emulation of lane groups (tests/test_hostsim_bot.py, which stays) and on the device, measured 1.9-2.4 x SLOWER than lane = env
// (profiles/r05/NOTES.md section 11); a 4-waves-per-SIMD build of it produced different decisions, never explained -- 250 KB of dead-by-default
// code with an open question attached does not belong in the product.
#ifndef BBAI_BOT_GROUP_BUILD
#define BBAI_BOT_GROUP_BUILD 0
#endif
#if BBAI_BOT_GROUP_BUILD

// The expert as ONE LANE GROUP PER ENV (G lanes, 64 / G envs per wave; bbai_bot.hpp "Execution model"): the subgoal machine runs
// group-uniform, the view, the mask rows, the neighbours of a popped position and the acceptance / key scans are split over the lanes.
// Per group in LDS: the four row-mask arrays [R_ALL][H], search 1's predecessor + queue arrays [2][W * H] uint16 (the eager first
// search never leaves LDS), and the env's BotState for the length of the decision (the subgoal stack stays in global memory: a
// decision touches its top).  Search 2's arrays (only when search 1 failed) are per-resident-group global scratch.
__host__ __device__ inline int botg_group_words(const LevelCfg& c) {
    return R_ALL * c.H + (2 * c.W * c.H * 2 + 3) / 4 + (int)sizeof(BotState) / 4;
}
template <int G, int WAVES_PER_SIMD>
__global__ __launch_bounds__(64, WAVES_PER_SIMD) void k_botg(LevelCfg c, int64_t n, const uint8_t* __restrict__ recs, const uint8_t* __restrict__ ring, int depth,
                                             const Hot* __restrict__ hots, const uint64_t* __restrict__ stales, uint8_t* __restrict__ states, int stack_cap,
                                             uint16_t* __restrict__ works, int eager, const uint8_t* __restrict__ prev_actions, uint8_t* __restrict__ out,
                                             unsigned long long* __restrict__ stats, int dead_action, uint8_t* __restrict__ gave_up) {
    extern __shared__ uint32_t s_botg[];
    constexpr int NG = 64 / G, SW = (int)sizeof(BotState) / 4;
    const GroupCtx<G> ctx;
    const int lane = ctx.lane();
    const int cells = c.W * c.H;
    uint32_t* blk = s_botg + ((int)threadIdx.x / G) * botg_group_words(c);
    const int64_t group = (int64_t)blockIdx.x * NG + (int)threadIdx.x / G, ngroups = (int64_t)gridDim.x * NG;
    BotWork w;
    w.eager = eager;
    w.ring = nullptr; w.ring_stride = 0; w.ring_size = 0;
    w.rows_fast = blk; w.rstride_fast = 1; w.rows_h = c.H; w.fast_n = R_ALL;
    w.rows_slow = nullptr; w.rstride_slow = 0;
    w.cells = cells;
    w.near_q = (uint16_t*)(blk + R_ALL * c.H);
    w.base = works + group * (int64_t)(4 * cells);          // (arrays 2, 3: search 2)
    w.stride = 1;
    uint32_t* sst = blk + R_ALL * c.H + (2 * cells * 2 + 3) / 4;
    BotState& st = *(BotState*)sst;
    const size_t sbytes = bot_state_bytes(stack_cap);
    for (int64_t i = group; i < n; i += ngroups) {
        const Hot h = hots[i];
        if (h.frozen) {
            if (lane == 0) { out[i] = A_DONE; if (gave_up) gave_up[i] = 0; }
            continue;
        }
        uint32_t* gst = (uint32_t*)(states + i * (int64_t)sbytes);
        for (int k = lane; k < SW; k += G) sst[k] = gst[k];
        ctx.sync();
        const bool first = h.step == 0 || st.next_step != h.step;
        const int taken = (prev_actions && !first) ? prev_actions[i] : -1;
        const bool was_dead = !first && st.dead;
        const int a = bot_decide(ctx, c, live_rec(c, n, i, (uint8_t*)recs, (uint8_t*)ring, depth, h.slot), h, stales[i], st, (Subgoal*)(gst + SW), stack_cap, w, first, taken);
        ctx.sync();
        if (lane == 0) {
            out[i] = (uint8_t)(a == BOT_DEAD ? dead_action : a);
            if (gave_up) gave_up[i] = a == BOT_DEAD ? 1 : 0;
            if (a == BOT_DEAD && !was_dead) atomicAdd(&stats[st.dead == DEAD_CAPACITY ? 1 : 0], 1ull);
        }
        for (int k = lane; k < SW; k += G) gst[k] = sst[k];
        ctx.sync();
    }
}
#endif
