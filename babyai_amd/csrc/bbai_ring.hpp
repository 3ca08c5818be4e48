// bbai_ring.hpp -- the look-ahead ring's turnover and the state's way in and out.
//   k_consume      wave = env over the reset list (unfused steps, reset()): look-ahead slot -> live state, SoA verifier view, first observation
//                  (consume_env, bbai_stepk.hpp: the stepping wave of a fused step does the same).
//   k_compact / k_mark / k_gate   the windows' turnover: the refill's work list (look-ahead stream), the refill's completion count, and
//                  the step stream's wait for "every env is sure to keep a window's worth of ready levels" (see NWIN, bbai_kernels.hpp).
//   k_probe_wait / k_probe_set   whether a caller's stream and the look-ahead stream make progress side by side (probe_stream).
//   k_live_copy / k_import_hot / k_sync_prog / k_sync_view / k_sync_cpl   export, import and checkpoints: the staged records and what is derived from them.
//   k_seed / k_init_hot   env.seed(s) and the empty state behind bbai_create.
// Part of bbai_engine.hip's translation unit: included where the code stood, at global scope.  The launches are bbai_engine.hip's.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include "bbai_types.hpp"
#include "bbai_kernels.hpp"
#include "bbai_step.hpp"
#include "bbai_seed.hpp"
#include "bbai_stepk.hpp"

using namespace bbai;

// look-ahead slot -> live state for the envs that finished (or all, on reset()): one wave copies one record
__global__ __launch_bounds__(256) void k_consume(LevelCfg c, int64_t n, uint8_t* recs, Hot* __restrict__ hots,
                                                 uint64_t* __restrict__ stales, uint8_t* next_recs,
                                                 const Hot* __restrict__ next_hots, uint32_t* __restrict__ vheads,
                                                 uint64_t* __restrict__ vsets, const int32_t* __restrict__ reset_list,
                                                 const uint8_t* __restrict__ reset_slot, const uint32_t* __restrict__ counter, int all,
                                                 unsigned long long* __restrict__ totals, int depth,
                                                 uint8_t* __restrict__ pending, uint8_t* __restrict__ first_slot,
                                                 uint32_t* __restrict__ win_meta,
                                                 uint8_t* __restrict__ image, uint8_t* __restrict__ dirs,
                                                 uint32_t* __restrict__ other_counter, int prio,
                                                 uint8_t* __restrict__ vplane /* or NULL */, uint16_t* __restrict__ fcache,
                                                 uint8_t* __restrict__ lsm_arr /* or NULL */, int inplace, uint8_t* __restrict__ cplane /* or NULL */) {
    if (prio) __builtin_amdgcn_s_setprio(3);
    const int64_t count = all ? n : (int64_t)counter[0];
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t it = wave; it < count; it += nwaves) {
        const int64_t env = all ? it : (int64_t)reset_list[it];
        const int slot = all ? (int)hots[env].slot : (int)reset_slot[it];       // (k_step listed it next to the env: no round trip through the env's state)
        consume_env(c, n, env, slot, lane, recs, hots, stales, next_recs, next_hots, vheads, vsets, depth, pending, first_slot,
                    win_meta, image + env * OBS_BYTES, dirs, vplane, fcache, lsm_arr, inplace != 0, cplane);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        atomicAdd(&totals[0], (unsigned long long)count);
        other_counter[0] = 0;       // the next step's k_step appends to the other ping-pong counter from zero
    }
}

// ---- window turnover (NWIN: bbai_kernels.hpp) ------------------------------------------------------------------------------------------------
// k_compact, look-ahead stream, in front of the window's k_pregen: the envs whose `pending` byte is set, as SHARDS dense sub-lists.  Wave
// w covers envs [64 w, 64 w + 64) and appends to sub-list w % SHARDS: one returning atomic per wave that found any, spread over SHARDS
// counters (1 048 576 envs, every one pending: 256 per counter) -- off the step path, a few microseconds per window.
__global__ __launch_bounds__(256) void k_compact(int64_t n, const uint8_t* __restrict__ pending, int32_t* __restrict__ gen_list, uint32_t* __restrict__ gen_count,
                                                 int64_t wave0, int64_t waves /* this look-ahead stream's 64-env blocks: [wave0, wave0 + waves) */) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = wave0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t env = wave * 64 + lane;
    const bool mine = wave < wave0 + waves && env < n && pending[env] != 0;
    const unsigned long long bal = __ballot(mine);
    if (!bal) return;
    const int j = (int)(wave % SHARDS);
    const int leader = __ffsll((long long)bal) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(&gen_count[j * GEN_COUNT_U32], (uint32_t)__popcll(bal));
    base = __shfl(base, leader);
    if (mine) gen_list[(int64_t)j * gen_sublist_cap(n) + base + __popcll(bal & ((1ull << lane) - 1ull))] = (int32_t)env;
}
// k_mark, look-ahead stream, behind the refill of window w: `refilled` = w + 1.  (A kernel of its own: the refill's stores are visible to
// whoever sees this value because that kernel has ENDED -- no fence inside the generator's waves.)
__global__ void k_mark(unsigned long long* __restrict__ flow, unsigned long long refilled) {
    __hip_atomic_store(&flow[FLOW_REFILLED], refilled, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
// k_gate, step stream, in front of the first tick of window x (which uses buffer x % NWIN): waits until
//   (a) the windows r .. x - 1 whose refill has not landed (r = `refilled`) are at most NWIN - 1 (buffer x % NWIN is free again), and
//   (b) the sum of their M (meta[0]; 1 unless an env finished repeatedly inside one window) is <= B: every env then has at least
//       2B - B = B ready levels, and window x consumes at most B per env;
// then clears the meta line of window x.  With r = x - 1 (rounds 1-4 waited for exactly that) both hold trivially, so the wait ends at the
// latest when refill x - 2 lands; every refill it can wait for was enqueued before it.  One wave; polls with s_sleep.  A wait beyond
// ~10 s of the constant 100-MHz clock gives up (counted in flow[FLOW_GATE_TIMEOUTS], read back as option "gate_timeouts": the handle's
// results are void then -- it means a lost refill, never seen) instead of hanging the device.
__global__ __launch_bounds__(64) void k_gate(unsigned long long* __restrict__ flow, uint32_t* __restrict__ metas, unsigned long long x, int period,
                                              uint32_t* __restrict__ host_fault /* pinned host word: sticky, read by every entry point */) {
    const int lane = (int)threadIdx.x;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        const unsigned long long r = __hip_atomic_load(&flow[FLOW_REFILLED], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long open = x > r ? x - r : 0ull;          // windows r .. x - 1
        uint32_t m = 0;
        if ((unsigned long long)lane < open && open < (unsigned long long)NWIN) {
            m = metas[(size_t)((r + lane) % NWIN) * META_U32];
            m = m < 1u ? 1u : m;
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) m += __shfl_xor(m, o);
        if (open < (unsigned long long)NWIN && m <= (uint32_t)period) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > 1000000000ull) {
            if (lane == 0) {
                atomicAdd(&flow[FLOW_GATE_TIMEOUTS], 1ull);
                __hip_atomic_store(host_fault, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            break;
        }
        __builtin_amdgcn_s_sleep(32);
    }
    if (lane == 0) metas[(size_t)(x % NWIN) * META_U32] = 0;
}

// probe_stream's two kernels: the waiter (caller's stream) polls a flag for at most ~20 ms of the 100-MHz clock, the setter (look-ahead stream, enqueued
// BEHIND it) raises it.  Verdict into pinned host memory: 1 = the setter ran while the waiter was resident (the streams are concurrent), 2 = it did not.
__global__ void k_probe_wait(unsigned long long* __restrict__ flow, uint32_t* __restrict__ host_verdict) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    uint32_t v = 2;
    for (;;) {
        if (__hip_atomic_load(&flow[FLOW_PROBE], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != 0ull) { v = 1; break; }
        if (__builtin_amdgcn_s_memrealtime() - t0 > 2000000ull) break;
        __builtin_amdgcn_s_sleep(16);
    }
    __hip_atomic_store(host_verdict, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void k_probe_set(unsigned long long* __restrict__ flow, unsigned long long v) {
    __hip_atomic_store(&flow[FLOW_PROBE], v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// In-place layout: rec[] is the staging area of export / import / checkpoints.  dir 0: live slots -> rec[first ..], dir 1: rec[first ..] -> live
// slots; one wave per env.
__global__ __launch_bounds__(256) void k_live_copy(LevelCfg c, int64_t n, int64_t first, int64_t count, uint8_t* __restrict__ recs,
                                                   uint8_t* __restrict__ ring, const Hot* __restrict__ hots, int depth, int dir) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const int nvec = c.rec_bytes >> 4;
    for (int64_t it = wave; it < count; it += nwaves) {
        const int64_t env = first + it;
        u32x4* stage = (u32x4*)(recs + env * (int64_t)c.rec_bytes);
        u32x4* live = (u32x4*)(ring + ring_at(live_slot(hots[env].slot, depth), env, depth) * (int64_t)c.rec_bytes);
        for (int k = lane; k < nvec; k += 64) { if (dir) live[k] = stage[k]; else stage[k] = live[k]; }
    }
}
// ... and an imported hot state keeps the env's place in its ring (hot.slot): the slot says where the live record IS
__global__ void k_import_hot(int64_t first, int64_t count, const Hot* __restrict__ staged, Hot* __restrict__ hots) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    Hot h = staged[i];
    h.slot = hots[first + i].slot;
    hots[first + i] = h;
}

// rebuild the SoA verifier view from the records (after bbai_import_state)
__global__ void k_sync_prog(LevelCfg c, int64_t n, int64_t first, int64_t count, const uint8_t* __restrict__ recs,
                            uint32_t* __restrict__ vheads, uint64_t* __restrict__ vsets) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int64_t env = first + i;
    const Prog* p = (const Prog*)(recs + env * (int64_t)c.rec_bytes + c.off_prog);
    for (int k = 0; k < 8; ++k) vsets[(int64_t)k * n + env] = p->set[k >> 1][k & 1];
    vheads[env] = vhead_pack(*p);
}

// rebuild the window plane and the front-cell cache from the live records (after bbai_import_state / checkpoint_load):
// one wave per env
__global__ __launch_bounds__(256) void k_sync_view(LevelCfg c, int64_t first, int64_t count, const uint8_t* __restrict__ recs,
                                                   const Hot* __restrict__ hots, uint8_t* __restrict__ vplane, uint16_t* __restrict__ fcache) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const int nseg = v_nxo(c) * v_nyo(c) * 8;
    for (int64_t it = wave; it < count; it += nwaves) {
        const int64_t env = first + it;
        const uint8_t* rec = recs + env * (int64_t)c.rec_bytes;
        uint8_t* vrow = vplane + env * (int64_t)v_bytes(c);
        for (int sg = lane; sg < nseg; sg += 64) *(u32x4*)(vrow + (sg >> 3) * VLINE + (sg & 7) * 16) = v_segment(c, rec, sg >> 3, sg & 7, -1);
        if (lane == 0) {
            const Hot h = hots[env];
            const uint32_t fe = rec[e_index(c, h.ax + dir_dx(h.dir), h.ay + dir_dy(h.dir))];
            const uint32_t ce = h.carry != NONE8 ? rec[c.off_app + h.carry] : (uint32_t)E_EMPTY;
            fcache[env] = (uint16_t)(fe | (ce << 8));
        }
    }
}

// ... and the C plane rows + the carried object's appearance of the small single rooms (in-place layout): one wave per env, from the staged records
__global__ __launch_bounds__(256) void k_sync_cpl(LevelCfg c, int64_t first, int64_t count, const uint8_t* __restrict__ recs,
                                                  const Hot* __restrict__ hots, uint8_t* __restrict__ cplane, uint16_t* __restrict__ fcache) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t it = wave; it < count; it += nwaves) {
        const int64_t env = first + it;
        const uint8_t* rec = recs + env * (int64_t)c.rec_bytes;
        cpl_build_wave(c, rec, cplane + env * (int64_t)cpl_bytes(c), lane);
        if (lane == 0) {
            const Hot h = hots[env];
            const uint32_t fe = rec[e_index(c, h.ax + dir_dx(h.dir), h.ay + dir_dy(h.dir))];
            const uint32_t ce = h.carry != NONE8 ? rec[c.off_app + h.carry] : (uint32_t)E_EMPTY;
            fcache[env] = (uint16_t)(fe | (ce << 8));
        }
    }
}

// env.seed(s) for every env: lane = env.  Each lane writes its own 624-word state (2496-byte pitch): a wave's 64 open
// lines stay in L2 until they are full, so HBM sees each state line once.
__global__ __launch_bounds__(64) void k_seed(int64_t n, const uint64_t* __restrict__ seeds, uint32_t* __restrict__ mts, int32_t* __restrict__ mtis) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    seed_env(seeds[i], mts + i * MT_N);
    mtis[i] = MT_N;                               // output index 624: the first draw twists (RandomState.seed leaves pos = N)
}

__global__ void k_init_hot(int64_t n, Hot* __restrict__ hots, Hot* __restrict__ next_hots, uint64_t* __restrict__ stales, int depth) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        Hot h;
        memset(&h, 0, sizeof(h));
        h.carry = NONE8; h.frozen = 1; h.last_locked = NONE8;
        h.pre4 = 0xFFFFFFFFu;
        hots[i] = h;
        for (int d = 0; d < depth; ++d) next_hots[ring_at(d, i, depth)] = h;
        stales[i] = 0;
    }
}
