// bbai_pregen.hpp -- the lane-group level generator and the canonical forms of the generators' RNG state.
//   k_pregen<F, G, OBS>  (F = level family) one env per group of G lanes: the NEXT levels of an env's MT19937 stream, working set in LDS
//                  (bbai_gen.hpp), into the env's look-ahead ring (OBS: + the level's first observation).  step() draws no randomness, so an
//                  env's level sequence is a pure function of its seed: generation runs ahead of need on a second HIP stream, one launch per
//                  window of B consume-ticks over the list k_compact builds from the window's `pending` bytes.
//   k_mt_sync / k_mt_canon   between the raw MT19937 words this kernel reads and the tempered generations k_pregen_lane reads
//                  (bbai_genlane.hip, bbai_genl.hpp).
// Part of bbai_engine.hip's translation unit: included where the code stood, at global scope.  The launches are bbai_engine.hip's
// (launch_pregen_g, mt_sync, mt_canon).
#pragma once
#include <hip/hip_runtime.h>
#include "bbai_types.hpp"
#include "bbai_kernels.hpp"
#include "bbai_gen.hpp"
#include "bbai_genl.hpp"
#include "bbai_step.hpp"

using namespace bbai;

// ------------------------------------------------------------------------------------------
// k_pregen / k_consume : look-ahead level generation (one wavefront generates one env's levels)
// ------------------------------------------------------------------------------------------
// One env per group of G lanes, 64 / G envs per wavefront (bbai_gen.hpp "Execution model").  sync() orders the group's LDS
// accesses: it is reached under divergent control flow (the groups of a wave are in different places of the generator),
// so it is a wave-local fence, never a workgroup barrier -- the workgroup is one wave.
// (GroupCtx<G>: bbai_kernels.hpp)

// (Lane = level -- GroupCtx<1>: the same templates with a one-lane context, working set in per-lane global memory, MT19937 state advanced in
// place -- was built and measured in round 5 (profiles/r05/NOTES.md): 86-95 VGPRs, but every access to the working set becomes a global
// round trip: bulk fill 2 x SLOWER (PickupLoc 7.4 -> 14.2 ns per level, GoTo 35 -> 82), in the step loop 2-7 x.  Removed.)
// The look-ahead generator.  A workgroup is ONE wave carrying 64 / G envs; every group walks its share of the window's `pending`
// bytes on its own: fetch an env that has levels pending, load its MT19937 state into the
// group's LDS block, then one ATTEMPT of the generator's rejection loop per trip of the main loop (Gen::attempt) -- a
// group whose attempt was accepted writes the level out and goes on to its next level / env while its neighbours retry,
// so the wave only idles lanes inside an attempt, never across attempts.
// Work list: the window's finished envs as SHARDS dense sub-lists (k_compact); entry k of their concatenation is found through the
// prefix of the sub-counts (64 words in LDS, a six-step search per entry: once per level, i.e. per ~50-300 us of work); groups stride
// over the entries, so every group gets the same number of envs to within one.  `dense` (bbai_seed's first fill): every env, no list.
// Minimum waves per SIMD the generator's register allocation has to allow.  4 (<= 128 VGPRs) instead of the 3 the compiler
// settles on by itself (131-135 VGPRs at two envs per wave): PickupLoc 262 144 envs 0.0939 -> 0.0877 ms per step, the GoTo family
// already fits (profiles/r04/pregen_waves_per_simd_ab.jsonl).  The bonus family would spill (167 VGPRs) and four envs per wave
// need 200: those keep 2.
#ifndef BBAI_PREGEN_WAVES
#define BBAI_PREGEN_WAVES 4
#endif
template <int KIND, int G, bool OBS /* in-place layout: the level's first observation is written next to it */>
__global__ __launch_bounds__(64, (KIND == K_BONUS || G == 16) ? 2 : BBAI_PREGEN_WAVES) void k_pregen(LevelCfg c, int64_t n, uint8_t* __restrict__ next_recs,
                                                  Hot* __restrict__ next_hots, uint32_t* __restrict__ mts,
                                                  int32_t* __restrict__ mtis,
                                                  const int32_t* __restrict__ gen_list, const uint32_t* __restrict__ gen_count /* NULL: dense -- every env, the whole grid works */,
                                                  int depth,
                                                  uint8_t* __restrict__ pending, const uint8_t* __restrict__ first_slot,
                                                  unsigned long long* __restrict__ gen_failures, int min_groups, int per_group /* list entries a working group should get */,
                                                  uint8_t* __restrict__ next_obs /* in-place layout: [D][n][OBS_SLOT], else NULL */) {
    constexpr int NG = 64 / G;
    typedef GroupCtx<G> Ctx;
    const Ctx ctx;
    __shared__ GenWork ws[NG];
    __shared__ uint32_t s_mt[NG][MT_N + MT_CH];      // the env's MT19937 state + the generator's chunk of tempered outputs (bbai_gen.hpp MT_CH)
    GenWork& w = ws[threadIdx.x / G];
    const int lane = ctx.lane();
    // the refill list: prefix of the sub-list lengths (one word per lane, a wave scan, parked in LDS for the groups' searches)
    __shared__ uint32_t s_start[SHARDS + 1];
    int64_t count = n;
    const int64_t cap = gen_sublist_cap(n);
    if (gen_count) {
        uint32_t c = gen_count[threadIdx.x * GEN_COUNT_U32], incl = c;            // (SHARDS == 64 == the block)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if ((int)threadIdx.x >= o) incl += t; }
        s_start[threadIdx.x + 1] = incl;
        if (threadIdx.x == 0) s_start[0] = 0;
        __syncthreads();
        count = (int64_t)s_start[SHARDS];
    }
    // How many lane groups WORK on a window's refill (single rooms): the grid is sized for the worst case (every env finished on every
    // tick), the list usually holds a fraction of that, and every resident generator wave holds registers and LDS that the step kernels'
    // workgroups queue for -- but a refill that takes as long as a window paces the whole step stream (k_gate).  active = entries /
    // per_group, at least `min_groups`, at most the grid; surplus blocks leave at once.  Round 4 (k_step + k_consume, 25 + 15 us per
    // step at 65 536 envs) found entries / 32 and >= 2 048 groups best.  Round 5, with k_step at 16 us, no second launch and the
    // stream free to run ahead of the refills, the SAME sweep says: more groups, shorter refills (profiles/r05/pregen_sizing_sweep.jsonl,
    // ms per step): GoToLocal 65 536 envs 0.0319 at 2 048 groups, 0.0205 at 4 096, 0.0179 at 6 144, 0.0199 at 8 192, 0.0206 with the whole grid;
    // GoToLocal 32 768: 0.0181 / 0.0122 / 0.0127 at 2 048 / 4 096 / 8 192; PickupLoc 262 144: 0.0755 at entries / 32, 0.067 at / 16, 0.059-0.063
    // at / 12 ... / 4; GoToLocal 262 144: 0.0706 / 0.0644 / 0.0618 / 0.0655 at / 32, 16, 8, 4; PickupLoc 524 288: 0.134 / 0.121 / 0.124 / 0.132.
    // Shipped: entries / 12, at least 6 144 groups.
    int64_t stride = (int64_t)gridDim.x * NG;
    if (gen_count && min_groups > 0) {
        int64_t active = count / per_group;
        active = active < min_groups ? min_groups : active;
        active = (active + NG - 1) / NG * NG;                   // whole blocks: every group of a block that stays has its own residue
        stride = active < stride ? active : stride;
    }
    int64_t it = (int64_t)blockIdx.x * NG + threadIdx.x / G;
    if ((int64_t)blockIdx.x * NG >= stride) return;             // (whole blocks only: the groups of a wave stay together)
    // the group's current env
    bool have = false;
    int64_t env = 0;
    int cnt = 0, done_levels = 0, slot = 0, mti = 0, last_locked = -1, attempts = 0;
    bool dirty = false;           // the env's state words were regenerated (a twist) since they were loaded: only then do they go back
    for (;;) {
        if (!have) {
            while (it < count) {
                int64_t cand = it;
                if (gen_count) {
                    // entry `it` of the concatenated sub-lists: the sub-list j with s_start[j] <= it < s_start[j + 1]
                    int j = 0;
#pragma unroll
                    for (int o = SHARDS / 2; o; o >>= 1) if ((int64_t)s_start[j + o] <= it) j += o;
                    cand = (int64_t)gen_list[(int64_t)j * cap + (it - (int64_t)s_start[j])];
                }
                it += stride;
                const int pc = pending[cand];            // levels to generate for this env (consecutive ring slots)
                if (pc == 0) continue;                   // (dense: env was not consumed in this window)
                env = cand; cnt = pc; have = true;
                break;
            }
            if (have) {
                // the env's generator state: all of its loads in flight together (MT19937 words, position, first slot) -- as a
                // load - store loop this was five dependent round trips before the first draw
                const uint32_t* mt = mts + env * MT_N;
                constexpr int MTQ = (MT_N + G - 1) / G;
                uint32_t mtw[MTQ];
#pragma unroll
                for (int q = 0; q < MTQ; ++q) { const int k = lane + q * G; mtw[q] = mt[k < MT_N ? k : MT_N - 1]; }
                mti = mtis[env];
                slot = first_slot[env];
                ctx.sync();
#pragma unroll
                for (int q = 0; q < MTQ; ++q) { const int k = lane + q * G; if (k < MT_N) s_mt[threadIdx.x / G][k] = mtw[q]; }
                ctx.sync();
                const int prev = slot == 0 ? depth - 1 : slot - 1;          // holds the level generated just before
                last_locked = next_hots[ring_at(prev, env, depth)].last_locked;   // LevelGen.locked_room survives episodes
                last_locked = last_locked == NONE8 ? -1 : last_locked;
                done_levels = 0; attempts = 0; dirty = false;
            }
        }
        if (__ballot(have) == 0ull) break;               // every group of the wave has run out of work
        if (!have) continue;
        Gen<Ctx> g(ctx, c, w, s_mt[threadIdx.x / G], s_mt[threadIdx.x / G] + MT_N, mti, last_locked);
        bool ok = g.template attempt<KIND>();
        mti = g.mti;
        dirty |= g.twisted;
        last_locked = g.last_locked;
        // last-resort guard (Gen::MAX_ATTEMPTS): never seen; keeps an impossible level from hanging the device
        const bool gave_up = !ok && ++attempts >= Gen<Ctx>::MAX_ATTEMPTS;
        if (!ok && !gave_up) continue;
        const int max_steps = g.finish();
        // write-out: record planes, tables, program
        uint8_t* rec = next_recs + ring_at(slot, env, depth) * (int64_t)c.rec_bytes;
        {
            const uint32_t* src = (const uint32_t*)w.E;
            uint32_t* dst = (uint32_t*)rec;
            const int ndw = (c.ES * c.EH) >> 2;
            for (int k = lane; k < ndw; k += G) dst[k] = src[k];
        }
        {
            const int cells = c.W * c.H, ndw = (cells + 3) >> 2;          // off_I is a dword multiple, the plane is padded to one
            const uint32_t* src = (const uint32_t*)w.I;
            uint32_t* dst = (uint32_t*)(rec + c.off_I);
            for (int k = lane; k < ndw; k += G) {
                uint32_t v = src[k];
                if (4 * k + 4 > cells) v &= 0xFFFFFFFFu >> (8 * (4 * k + 4 - cells));      // bytes past the plane stay zero
                dst[k] = v;
            }
        }
        for (int k = lane; k < c.maxo; k += G) {
            bool used = k < g.nobj;
            rec[c.off_app + k] = used ? w.app[k] : 0;
            rec[c.off_pos + 2 * k] = used ? w.px[k] : 0;
            rec[c.off_pos + 2 * k + 1] = used ? w.py[k] : 0;
            rec[c.off_cont + k] = used ? w.cont[k] : NONE8;
        }
        {
            const uint32_t* src = (const uint32_t*)&w.prog;
            uint32_t* dst = (uint32_t*)(rec + c.off_prog);
            for (int k = lane; k < (int)(sizeof(Prog) / 4); k += G) dst[k] = src[k];
        }
        if constexpr (OBS) {
            // In-place layout: the level's first observation (gen_obs at the start pose: MiniGridEnv.reset), from the appearance plane
            // in LDS.  Lane l of the group takes view cells l, l + G, ...: cell = vi + 7 vj; the opacity mask of the view is the
            // group's share of a ballot per round; every lane runs the 7-row visibility sweep and writes its cells' three bytes
            // (the layout observe_emit writes: cell (vi, vj) at byte (7 vi + vj) * 3; the agent's own cell shows what it carries: nothing yet).
            uint8_t* ob = next_obs + ring_at(slot, env, depth) * OBS_SLOT;
            constexpr int R = (VIEW * VIEW + G - 1) / G;
            constexpr unsigned long long GM = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
            int ec[R];
            unsigned long long opaque = 0;
            ctx.sync();
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int cell = r * G + lane;
                int e = E_EMPTY;
                if (cell < VIEW * VIEW) {
                    int x, y;
                    view_to_world(g.ax, g.ay, g.adir, cell % VIEW, cell / VIEW, x, y);
                    e = w.E[(y + MARGIN) * c.ES + (x + MARGIN)];
                }
                ec[r] = e;
                const unsigned long long bal = __ballot(cell < VIEW * VIEW && e_opaque(e));
                opaque |= ((bal >> ((int)threadIdx.x & ~(G - 1) & 63)) & GM) << (r * G);
            }
            uint32_t opq[VIEW], vis[VIEW];
#pragma unroll
            for (int r = 0; r < VIEW; ++r) opq[r] = (uint32_t)(opaque >> (VIEW * r)) & 0x7Fu;
            process_vis_rows(opq, vis);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int cell = r * G + lane;
                if (cell < VIEW * VIEW) {
                    const int vi = cell % VIEW, vj = cell / VIEW;
                    const int e = (vi == 3 && vj == 6) ? (int)E_EMPTY : ec[r];
                    uint32_t row = 0;
#pragma unroll
                    for (int q = 0; q < VIEW; ++q) row = (vj == q) ? vis[q] : row;
                    const bool v = row >> vi & 1;
                    uint8_t* o = ob + (vi * VIEW + vj) * 3;
                    o[0] = v ? e_type(e) : 0; o[1] = v ? e_color(e) : 0; o[2] = v ? e_state(e) : 0;
                }
            }
            // ... and, for the small single rooms, the level's C plane row (bbai_types.hpp): the grid at pitch 8 + where every object stands
            if (cpl_ok(c)) {
                uint8_t* row = ob + CPL_OFF;
                for (int d = lane; d < CPL_PLANE / 4; d += G) {
                    const int y = d >> 1, x0 = (d & 1) * 4;
                    uint32_t v = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int x = x0 + b;
                        const uint32_t e = (x < c.W && y < c.H) ? (uint32_t)w.E[(y + MARGIN) * c.ES + (x + MARGIN)] : (uint32_t)E_WALL;
                        v |= e << (8 * b);
                    }
                    ((uint32_t*)row)[d] = v;
                }
                for (int k = lane; k < CPL_MAX_IDS; k += G)
                    row[CPL_PLANE + k] = (k < g.nobj && w.px[k] != NONE8) ? (uint8_t)(w.py[k] << 3 | w.px[k]) : (uint8_t)0xFF;
            }
        }
        if (lane == 0) {
            Hot h;
            h.ax = (uint8_t)g.ax; h.ay = (uint8_t)g.ay; h.dir = (uint8_t)g.adir; h.carry = NONE8;
            h.step = 0; h.max_steps = (uint16_t)max_steps;
            h.pre4 = 0xFFFFFFFFu;
            h.vstate = 0; h.frozen = 0;
            if (gave_up) {
                h.frozen = 2;
                atomicAdd(gen_failures, 1ull);
            }
            h.last_locked = last_locked < 0 ? NONE8 : (uint8_t)last_locked;
            h.slot = 0;
            next_hots[ring_at(slot, env, depth)] = h;
        }
        slot = slot + 1 == depth ? 0 : slot + 1;
        attempts = 0;
        if (++done_levels == cnt) {                      // this env's levels are done: MT state back, buffer entry free
            // draws only advance the index: the 624 state words change at a twist alone (every 624 draws -- one single-room level in seven)
            if (dirty) {
                uint32_t* mt = mts + env * MT_N;
                ctx.sync();
                for (int k = lane; k < MT_N; k += G) mt[k] = s_mt[threadIdx.x / G][k];
            }
            if (lane == 0) {
                mtis[env] = mti;
                pending[env] = 0;                        // buffer entry is free for a later window
            }
            have = false;
        }
    }
}

// Derived / canonical forms of the lane generator's RNG state.
//   k_mt_sync:  after anything that wrote (mts, mtis) in the canonical form (imports, checkpoint loads, the lane-group generator): the latest
//               generation's tempered outputs into half 0, parity 0.
//   k_mt_canon: before anything that reads the canonical form (checkpoint saves, the lane-group generator): an env whose position lies in
//               the PREVIOUS generation gets that generation's raw words back (un-tempered from its half) and position + 624.
__global__ __launch_bounds__(256) void k_mt_sync(int64_t n, const uint32_t* __restrict__ mts, uint32_t* __restrict__ mtt, uint8_t* __restrict__ mtpar) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * MT_N) return;
    const int64_t env = i / MT_N;
    const int k = (int)(i - env * MT_N);
    mtt[env * (2 * MT_N) + k] = mt_temper(mts[i]);
    if (k == 0) mtpar[env] = 0;
}
__global__ __launch_bounds__(256) void k_mt_canon(int64_t n, uint32_t* __restrict__ mts, uint32_t* __restrict__ mtt, uint8_t* __restrict__ mtpar, int32_t* __restrict__ mtis) {
    // one wave per env (the position is read by every lane before lane 0 rewrites it: the wave runs in lockstep up to the barrier)
    const int64_t env = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (env >= n) return;
    const int pos = mtis[env];
    const int par = mtpar[env];
    __builtin_amdgcn_wave_barrier();
    if (pos >= 0) return;
    const uint32_t* prev = mtt + env * (2 * MT_N) + (par ^ 1) * MT_N;
    for (int k = lane; k < MT_N; k += 64) mts[env * MT_N + k] = mt_untemper(prev[k]);
    if (lane == 0) { mtis[env] = pos + MT_N; mtpar[env] = (uint8_t)(par ^ 1); }
}
