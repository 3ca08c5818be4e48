// bbai_statek.hpp -- device snapshots: the live state of LISTED envs out of a handle and back into one, without a host trip.
//   k_state_save    wave = list entry: env ids[k] -> snapshot row k (record, hot state, stale set, lastStepMatch byte).
//   k_state_load    wave = list entry: snapshot row rows[k] -> env ids[k]: the live record, the hot state (the env keeps its own place in its ring,
//                   k_import_hot's rule), stale set and lastStepMatch byte; everything derived from the record, as the k_sync_* kernels
//                   (bbai_ring.hpp) build it -- verifier view, window plane, C plane row, front cache; the observation of the loaded state
//                   (observe_fetch / observe_emit, bbai_stepk.hpp); and an expert plan that no longer matches any step.
//   k_state_tokens  lane = list entry: the mission tokens of the loaded envs (k_tokens' sentence, bbai_tokens.hpp).
// The live state ONLY: neither kernel is a consume-tick -- the look-ahead ring, the windows' bookkeeping (pending, first_slot, win_meta, flow), the
// RNG streams and the gate are neither read nor written, so a restored env goes on with its own next level when the restored episode ends.
// Grids follow the list's length, never the batch's.  No LDS, no scratch (like k_consume: LDS would make the blocks queue behind the generator's).
// Part of bbai_engine.hip's translation unit: included behind the other families, at global scope.  The launches are bbai_engine.hip's
// (bbai_save_state, bbai_load_state).
// The three kernels are templates (one instantiation each, <0>) for the sake of where their code lands: a template's code is emitted where it is first
// launched, and bbai_save_state / bbai_load_state close bbai_engine.hip -- so the new kernels lie BEHIND every earlier kernel in the code object, and
// every earlier kernel keeps the place it had.  (As plain kernels they were emitted in front of all the templated ones -- k_step, k_render, k_pregen --
// whose code moved by their size: the headline measured 4 % slower against identical instructions, profiles/state_snapshot/README.md.)
#pragma once
#include <hip/hip_runtime.h>
#include "bbai_types.hpp"
#include "bbai_kernels.hpp"
#include "bbai_step.hpp"
#include "bbai_stepk.hpp"
#include "bbai_bot.hpp"
#include "bbai_tokens.hpp"

using namespace bbai;

// A record is 1.3 - 1.8 KB = at most STATE_CPB 16-byte vectors per lane of the wave that moves it: all of them are loaded before the first is stored.
constexpr int STATE_CPB = 2;
constexpr int STATE_MAX_REC = 64 * 16 * STATE_CPB;       // bbai_save_state / bbai_load_state refuse a level whose record is larger (none is)

__device__ __forceinline__ void state_rec_load(const uint8_t* __restrict__ src, int nvec, int lane, u32x4* buf) {
    const u32x4* s = (const u32x4*)src;
#pragma unroll
    for (int j = 0; j < STATE_CPB; ++j) buf[j] = s[lane + 64 * j < nvec ? lane + 64 * j : nvec - 1];
}
__device__ __forceinline__ void state_rec_store(uint8_t* __restrict__ dst, int nvec, int lane, const u32x4* buf) {
    u32x4* d = (u32x4*)dst;
#pragma unroll
    for (int j = 0; j < STATE_CPB; ++j) if (lane + 64 * j < nvec) d[lane + 64 * j] = buf[j];
}

template <int TAIL = 0>
__global__ __launch_bounds__(256) void k_state_save(LevelCfg c, int64_t n, const int64_t* __restrict__ ids /* or NULL: env k */, int64_t count,
                                                    uint8_t* recs, uint8_t* ring /* in-place layout, else NULL */, int depth,
                                                    const Hot* __restrict__ hots, const uint64_t* __restrict__ stales, const uint8_t* __restrict__ lsm_arr /* or NULL */,
                                                    uint8_t* __restrict__ rec_out, u32x4* __restrict__ hot_out, uint64_t* __restrict__ stale_out,
                                                    uint8_t* __restrict__ lsm_out /* or NULL */) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const int nvec = c.rec_bytes >> 4;
    for (int64_t k = wave; k < count; k += nwaves) {
        const int64_t env = ids ? ids[k] : k;
        if (env < 0 || env >= n) continue;
        const u32x4 hv = *(const u32x4*)(hots + env);
        const uint64_t st = stales[env];
        const uint8_t lm = lsm_arr ? lsm_arr[env] : (uint8_t)0;
        Hot h;
        __builtin_memcpy(&h, &hv, sizeof(h));
        u32x4 buf[STATE_CPB];
        state_rec_load(live_rec(c, n, env, recs, ring, depth, h.slot), nvec, lane, buf);
        asm volatile("" : "+v"(buf[0]), "+v"(buf[1]));       // (both loads in flight before the first store, as in consume_env)
        state_rec_store(rec_out + k * (int64_t)c.rec_bytes, nvec, lane, buf);
        if (lane == 0) {
            hot_out[k] = hv;
            stale_out[k] = st;
            if (lsm_out) lsm_out[k] = lm;
        }
    }
}

template <int TAIL = 0>
__global__ __launch_bounds__(256) void k_state_load(LevelCfg c, int64_t n, const int64_t* __restrict__ ids /* or NULL: env k */,
                                                    const int64_t* __restrict__ rows /* or NULL: row k */, int64_t count, int64_t snap_rows,
                                                    const uint8_t* __restrict__ rec_in, const u32x4* __restrict__ hot_in, const uint64_t* __restrict__ stale_in,
                                                    const uint8_t* __restrict__ lsm_in /* or NULL: zeros */,
                                                    uint8_t* recs, uint8_t* ring /* in-place layout, else NULL */, int depth,
                                                    Hot* __restrict__ hots, uint64_t* __restrict__ stales, uint8_t* __restrict__ lsm_arr /* or NULL */,
                                                    uint32_t* __restrict__ vheads, uint64_t* __restrict__ vsets,
                                                    uint8_t* __restrict__ vplane /* or NULL */, uint8_t* __restrict__ cplane /* or NULL */, uint16_t* __restrict__ fcache,
                                                    uint8_t* __restrict__ bot_states /* or NULL */, int bot_stack,
                                                    uint8_t* __restrict__ image, uint8_t* __restrict__ dirs) {
    static_assert(sizeof(Hot) == 16, "the hot state moves as one vector");
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const int nvec = c.rec_bytes >> 4;
    for (int64_t k = wave; k < count; k += nwaves) {
        const int64_t env = ids ? ids[k] : k;
        const int64_t row = rows ? rows[k] : k;
        if (env < 0 || env >= n || row < 0 || row >= snap_rows) continue;
        // everything below is derived from the snapshot row, which this kernel only reads: the loads depend on nothing the wave stores
        const uint8_t* src = rec_in + row * (int64_t)c.rec_bytes;
        const u32x4 hv = hot_in[row];
        const uint64_t st = stale_in[row];
        const uint8_t lm = lsm_in ? lsm_in[row] : (uint8_t)0;
        const int own_slot = hots[env].slot;                       // the ring belongs to the handle: the env keeps its place in it (k_import_hot)
        Hot h;
        __builtin_memcpy(&h, &hv, sizeof(h));
        h.slot = (uint8_t)own_slot;
        const Prog* p = (const Prog*)(src + c.off_prog);
        const uint64_t pset = lane < 8 ? p->set[lane >> 1][lane & 1] : 0ull;
        const uint32_t vh = vhead_pack(*p);
        const int e_view = observe_fetch(c, src, h, lane);
        const uint32_t fe = src[e_index(c, h.ax + dir_dx(h.dir), h.ay + dir_dy(h.dir))];
        const uint32_t ce = h.carry != NONE8 ? src[c.off_app + h.carry] : (uint32_t)E_EMPTY;
        u32x4 buf[STATE_CPB];
        state_rec_load(src, nvec, lane, buf);
        asm volatile("" : "+v"(buf[0]), "+v"(buf[1]));
        state_rec_store(live_rec(c, n, env, recs, ring, depth, own_slot), nvec, lane, buf);
        if (vplane) {          // the window plane of the loaded record (k_sync_view)
            uint8_t* vrow = vplane + env * (int64_t)v_bytes(c);
            const int nseg = v_nxo(c) * v_nyo(c) * 8;
            constexpr int SGB = 4;
            for (int s0 = lane; s0 < nseg; s0 += 64 * SGB) {
                u32x4 seg[SGB];
#pragma unroll
                for (int j = 0; j < SGB; ++j) { const int sg = s0 + 64 * j < nseg ? s0 + 64 * j : nseg - 1; seg[j] = v_segment(c, src, sg >> 3, sg & 7, -1); }
#pragma unroll
                for (int j = 0; j < SGB; ++j) { const int sg = s0 + 64 * j; if (sg < nseg) *(u32x4*)(vrow + (sg >> 3) * VLINE + (sg & 7) * 16) = seg[j]; }
            }
        }
        if (cplane) cpl_build_wave(c, src, cplane + env * (int64_t)cpl_bytes(c), lane);      // (k_sync_cpl)
        if (lane < 8) vsets[(int64_t)lane * n + env] = pset;                                 // (k_sync_prog)
        if (lane == 8) vheads[env] = vh;
        observe_emit(c, src, h, e_view, image + env * OBS_BYTES, lane);                      // gen_obs() of the loaded state
        if (lane == 0) {
            if (vplane || cplane) fcache[env] = (uint16_t)(fe | (ce << 8));
            hots[env] = h;
            stales[env] = st;
            if (lsm_arr) lsm_arr[env] = lm;
            dirs[env] = h.dir;
            // the expert's plan is not part of a snapshot: 0 is no step a plan can expect (k_bot starts a fresh Bot at step 0 anyway), so the
            // env's next decision starts one
            if (bot_states) ((BotState*)(bot_states + env * (int64_t)bot_state_bytes(bot_stack)))->next_step = 0;
        }
    }
}

// the registered token rows of the loaded envs: k_tokens' sentence for the listed envs only, behind k_state_load on the same stream
template <int TAIL = 0>
__global__ __launch_bounds__(64) void k_state_tokens(LevelCfg c, int64_t n, const int64_t* __restrict__ ids /* or NULL: env k */,
                                                     const int64_t* __restrict__ rows /* or NULL */, int64_t count, int64_t snap_rows,
                                                     const uint8_t* __restrict__ recs, const uint8_t* __restrict__ ring, int depth,
                                                     const Hot* __restrict__ hots, uint8_t* __restrict__ tokens) {
    for (int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x; k < count; k += (int64_t)gridDim.x * 64) {
        const int64_t env = ids ? ids[k] : k;
        const int64_t row = rows ? rows[k] : k;
        if (env < 0 || env >= n || row < 0 || row >= snap_rows) continue;          // (an entry k_state_load skipped)
        const Prog* p = (const Prog*)(live_rec(c, n, env, (uint8_t*)recs, (uint8_t*)ring, depth, ring ? hots[env].slot : 0) + c.off_prog);
        TokOut o; o.p = tokens + env * TOK_MAX; o.n = 0;
        tok_side(o, p, 0, p->n_a);
        if (p->root == R_BEFORE) { o.put(31); tok_side(o, p, 2, p->n_b); }
        else if (p->root == R_AFTER) { o.put(32); o.put(24); tok_side(o, p, 2, p->n_b); }
        while (o.n < TOK_MAX) o.p[o.n++] = 0;
    }
}
