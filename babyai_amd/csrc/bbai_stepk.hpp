// bbai_stepk.hpp -- the step kernels: k_step<VP, FUSE, CP> (one tick) and k_step_ticks (several ticks of a rollout in one launch), both around
// step_body, with what a stepping wave does for an env whose episode is over (consume_env, advance_load / advance_finish) and the dirty
// cells a step leaves for its delta render (step_dirty).
//   k_step<VP, FUSE>  lane = env, one wave per block.  Coalesced SoA loads of the 16-byte hot state, action, stale set and verifier program;
//                  per-lane transition + verifier on the env's record; the 7x7 window is fetched as 7 rows x 3 dwords (one 128-byte line
//                  of the window plane, VP) and rotated, occluded and masked in REGISTERS (bbai_view.hpp: byte permutes, SWAR opacity,
//                  dot-product row masks); the 147-byte encodings of the block's 64 envs are staged in LDS at the output pitch and leave as one
//                  contiguous 16-byte-per-lane span.  Finished envs: FUSE 1 -- the stepping wave consumes their look-ahead slots itself
//                  (consume_env); FUSE 3 (in-place layout) -- every finished lane moves its own env on to its next ring slot
//                  (advance_load / advance_finish); FUSE 0 -- compacted into a reset list for k_consume.  The fused paths leave NO
//                  returning atomic and no list behind: one fire-and-forget add to a sharded total per wave, per-env bytes for the refill.
// Part of bbai_engine.hip's translation unit: included where the code stood, at global scope (the resource report, bench.py and the
// profile tools find the kernels by their bare names).  The launches are bbai_engine.hip's (step_kernel).
#pragma once
#include <hip/hip_runtime.h>
#include "bbai_types.hpp"
#include "bbai_kernels.hpp"
#include "bbai_step.hpp"
#include "bbai_view.hpp"
#include "bbai_dirty.hpp"

using namespace bbai;

// ------------------------------------------------------------------------------------------
// k_step
// ------------------------------------------------------------------------------------------
// What a stepping wave leaves of its finished envs in the fused paths (the windows' bookkeeping, bbai_kernels.hpp): one add to its shard of the total.
__device__ __forceinline__ void count_resets(unsigned long long* __restrict__ totals, unsigned int k, unsigned int blk) {
    atomicAdd(&totals[(blk & (SHARDS - 1)) * SHARD_U64], (unsigned long long)k);        // (result unused: a no-return atomic)
}
// envs (= threads) per k_step block.  The kernel is bound by its chain of dependent memory round trips, not by bytes or
// instructions, and a block is what waits at its barriers for its slowest wave: ONE wave per block (64) measured against
// 128 / 256 in round 3 (profiles/r03/step_variants_ab.jsonl: BossLevel encoded 1 048 576 envs k_step 0.130 -> 0.124 -> 0.111 ms,
// PickupLoc 262 144 0.071 -> 0.061 -> 0.051, GoTo 131 072 0.0212 -> 0.0192 -> 0.0184, GoToLocal 65 536 0.0244 -> 0.0216 -> 0.0214).
// The in-wave consume (FUSE) RELIES on it: the LDS traffic of a block is ordered by the wave's program order alone.
constexpr int STEP_BLOCK = 64;
#ifndef BBAI_STEP_WAVES
#define BBAI_STEP_WAVES 1          // minimum waves per SIMD the register allocation of k_step has to allow (the compiler's own figures:
#endif                             // babyai_amd/kernel_resources.json, quoted in DESIGN.md section 4; the block's 9.4 KB of LDS stop at 17 blocks per CU)
// BBAI_PREFETCH_ID=1 (experiment): the id-plane entry of the front cell fetched WITH the window.  Measured slower everywhere
// (step_variants_ab.jsonl: BossLevel encoded 1M k_step 0.130 -> 0.148 ms, GoTo 131 072 0.021 -> 0.028): one more line per
// env-step costs more than the verifier's occasional extra round trip.  Off.
#ifndef BBAI_PREFETCH_ID
#define BBAI_PREFETCH_ID 0
#endif

// BBAI_VIEW_LDS=1 (A/B builds): rounds 2-4's view -- the window parked in LDS and read back cell by cell (view_cells / encode_view below).  The shipped
// path is bbai_view.hpp: the same view as byte permutes on packed registers (k_step: -~900 of ~2 600 vector instructions, -63 LDS operations per env-step).
#ifndef BBAI_VIEW_LDS
#define BBAI_VIEW_LDS 0
#endif
// Observation with the 7x7 window staged in LDS (rounds 2-4's k_step path).  49 scattered byte loads per lane keep the
// texture-address unit busy for most of k_step (tools/step_ab.py ablation), so the window is fetched in WORLD
// orientation as 7 rows x 3 aligned dwords, byte-aligned with v_alignbyte, parked in 56 dword-aligned bytes inside the
// lane's own LDS obs row (`scr`, bbai_step.hpp row_scratch), and read back in VIEW orientation (rotation = per-direction
// address arithmetic on ds_read_u8).  All of a lane's reads precede its writes and lanes only touch bytes of their own
// row, so no barrier is needed here.
// The window's rows come from `q` (first aligned dword of row 0), `rstride` dwords apart, `off` = byte offset of the
// window's first column inside that dword: the record's appearance plane (rstride = ES / 4) or the env's V-plane line
// (rstride = 4).  `ce` = appearance of what the agent carries (E_EMPTY: nothing).  `fe2` receives the appearance of the
// cell in front of the agent (view cell (3, 5)) for the verifier and the next step's transition.
// Two halves, so that the verifier (which only needs fe2) can run between them while nothing of the 37-dword encoding is
// live yet: view_cells fetches and rotates the window (cp = the 49 cells, vis = visibility rows), encode_view writes the
// encoding from them.
// window_fetch issues the loads (7 rows x 3 dwords: one dwordx3 each); view_cells consumes them.  k_step puts the rare
// object actions (pickup / drop / toggle: dependent record loads and stores) BETWEEN the two, so their memory round trips
// overlap the window's instead of preceding it.  Such an action changes exactly one cell of the window that was fetched
// before it ran -- the one in front of the agent, view cell (3, 5): `nfe` >= 0 is its new appearance, patched in LDS.
__device__ __forceinline__ void window_fetch(const uint32_t* __restrict__ q, int rstride, uint32_t* wd) {
#pragma unroll
    for (int r = 0; r < VIEW; ++r) { wd[3 * r] = q[r * rstride]; wd[3 * r + 1] = q[r * rstride + 1]; wd[3 * r + 2] = q[r * rstride + 2]; }
}
__device__ __forceinline__ void view_cells(const uint32_t* wd, int off, int dir, uint32_t ce, int nfe,
                                           uint8_t* __restrict__ scr /* this lane's 56 bytes of LDS scratch */, uint32_t* cp, uint32_t* vis, int& fe2) {
    uint32_t* win = (uint32_t*)scr;                          // 7 rows x 8 bytes, dword aligned
#pragma unroll
    for (int r = 0; r < VIEW; ++r) {
        win[2 * r] = __builtin_amdgcn_alignbyte(wd[3 * r + 1], wd[3 * r], off);
        win[2 * r + 1] = __builtin_amdgcn_alignbyte(wd[3 * r + 2], wd[3 * r + 1], off);
    }
    // view (vi, vj) -> window byte: dir3 (vj, vi), dir0 (vi, 6-vj), dir1 (6-vj, 6-vi), dir2 (6-vi, vj); row pitch 8
    const int k0 = dir == 0 ? 6 : dir == 1 ? 54 : dir == 2 ? 48 : 0;
    const int kvi = dir == 0 ? 8 : dir == 1 ? -1 : dir == 2 ? -8 : 1;
    const int kvj = dir == 0 ? -1 : dir == 1 ? -8 : dir == 2 ? 1 : 8;
    uint8_t* wb = scr + k0;
    if (nfe >= 0) wb[kvi * 3 + kvj * 5] = (uint8_t)nfe;      // (same lane: LDS operations of a lane stay in order)
#pragma unroll
    for (int k = 0; k < 13; ++k) cp[k] = 0;                      // the 49 cells, 4 per dword, view order [vi][vj]
    uint32_t opq[VIEW] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int vi = 0; vi < VIEW; ++vi)
#pragma unroll
        for (int vj = 0; vj < VIEW; ++vj) {
            const int idx = vi * VIEW + vj;
            const uint32_t e = wb[kvi * vi + kvj * vj];
            cp[idx >> 2] |= e << (8 * (idx & 3));
            opq[vj] |= (e_opaque((int)e) ? 1u : 0u) << vi;
        }
    process_vis_rows(opq, vis);
    fe2 = (int)((cp[(3 * VIEW + 5) >> 2] >> (8 * ((3 * VIEW + 5) & 3))) & 0xFFu);
    {   // the agent's own cell (3,6) shows what it carries
        constexpr int idx = 3 * VIEW + 6;
        cp[idx >> 2] = (cp[idx >> 2] & ~(0xFFu << (8 * (idx & 3)))) | (ce << (8 * (idx & 3)));
    }
}
// Four cells at a time: a dword of (visibility-masked) appearance bytes e0..e3 becomes the 12 encoding bytes
// t0 c0 s0 t1 | c1 s1 t2 c2 | s2 t3 c3 s3 (type = e & 7, colour = (e >> 3) & 7, state = e >> 6) with three field extractions on
// the whole dword and six byte permutes (v_perm_b32: selector bytes 0-3 pick from the second operand, 4-7 from the first,
// 0x0C is zero) -- 11 instructions per four cells instead of ~55 shifting every channel byte into place on its own.
__device__ __forceinline__ void encode_view(const uint32_t* cp, const uint32_t* vis, RowPacker o) {
#pragma unroll
    for (int k = 0; k < 13; ++k) {
        // the cells of this dword that are visible: byte b <- bit (idx / 7) of vis[idx % 7], idx = 4k + b
        uint32_t m = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int idx = 4 * k + b;
            if (idx < VIEW * VIEW) m |= (uint32_t)__builtin_amdgcn_sbfe((int)vis[idx % VIEW], idx / VIEW, 1) & (0xFFu << (8 * b));   // v_bfe_i32: 0 / ~0
        }
        const uint32_t x = cp[k] & m;
        const uint32_t t = x & 0x07070707u, c = (x >> 3) & 0x07070707u, st = (x >> 6) & 0x03030303u;
        if (k < 12) {
            o.put(3 * k, __builtin_amdgcn_perm(__builtin_amdgcn_perm(t, c, 0x050C0004u), st, 0x07000504u));
            o.put(3 * k + 1, __builtin_amdgcn_perm(__builtin_amdgcn_perm(c, st, 0x060C0105u), t, 0x07020504u));
            o.put(3 * k + 2, __builtin_amdgcn_perm(__builtin_amdgcn_perm(st, t, 0x070C0306u), c, 0x07030504u));
        } else {
            o.put(36, (t & 0xFFu) | ((c & 0xFFu) << 8) | ((st & 0xFFu) << 16));   // cell 48: three bytes, the row's last dword
        }
    }
    o.finish();
}

// Wave-cooperative observation of ONE env (used where a wave owns an env: consume_env): lane l < 49 owns view cell
// (vi, vj) = (l % 7, l / 7); the opacity mask of the whole view is one ballot; every lane runs the 7-row
// visibility sweep on it and writes its own three bytes.  In two halves so that the caller can put other memory traffic
// between the cell load and its use: observe_fetch returns the lane's cell, observe_emit does the rest.
__device__ __forceinline__ int observe_fetch(const LevelCfg& c, const uint8_t* __restrict__ rec, const Hot& h, int lane) {
    const int vi = lane % VIEW, vj = lane / VIEW;
    int e = E_EMPTY;
    if (lane < VIEW * VIEW) {
        int x, y;
        view_to_world(h.ax, h.ay, h.dir, vi, vj, x, y);
        e = rec[e_index(c, x, y)];
    }
    return e;
}
__device__ __forceinline__ void observe_emit(const LevelCfg& c, const uint8_t* __restrict__ rec, const Hot& h, int e,
                                             uint8_t* __restrict__ dst, int lane) {
    const int vi = lane % VIEW, vj = lane / VIEW;
    const unsigned long long opaque = __ballot(lane < VIEW * VIEW && e_opaque(e));
    uint32_t opq[VIEW], vis[VIEW];
#pragma unroll
    for (int r = 0; r < VIEW; ++r) opq[r] = (uint32_t)(opaque >> (VIEW * r)) & 0x7Fu;
    process_vis_rows(opq, vis);
    if (lane < VIEW * VIEW) {
        if (vi == 3 && vj == 6) e = h.carry != NONE8 ? rec[c.off_app + h.carry] : (int)E_EMPTY;
        uint32_t row = 0;
#pragma unroll
        for (int r = 0; r < VIEW; ++r) row = (vj == r) ? vis[r] : row;
        const bool v = row >> vi & 1;
        uint8_t* o = dst + (vi * VIEW + vj) * 3;
        o[0] = v ? e_type(e) : 0; o[1] = v ? e_color(e) : 0; o[2] = v ? e_state(e) : 0;
    }
}

// V-plane helpers (bbai_types.hpp "window plane").  Patch one cell into every line that holds it.
__device__ __forceinline__ void v_patch(const LevelCfg& c, uint8_t* __restrict__ vrow, int x, int y, int val) {
    const int xm = x + MARGIN, ym = y + MARGIN, nxo = v_nxo(c), nyo = v_nyo(c);
    const int yo_lo = ym >= 6 ? (ym - 6) >> 1 : 0, yo_hi = (ym >> 1) < nyo - 1 ? (ym >> 1) : nyo - 1;
    for (int xo = (xm >> 3) - 1; xo <= (xm >> 3); ++xo) {
        if (xo < 0 || xo >= nxo) continue;
        for (int yo = yo_lo; yo <= yo_hi; ++yo) vrow[(yo * nxo + xo) * VLINE + (ym - 2 * yo) * 16 + (xm - 8 * xo)] = (uint8_t)val;
    }
}
// One 16-byte row segment of a V-plane line out of an appearance plane (`E`, row pitch ES); `sc` = plane index of a cell
// to show as empty (the start-carry object, which leaves the grid right after the first observation), or -1.
__device__ __forceinline__ u32x4 v_segment(const LevelCfg& c, const uint8_t* __restrict__ E, int line, int r, int sc) {
    const int nxo = v_nxo(c);
    const int yo = line / nxo, xo = line - yo * nxo;
    const int prow = 2 * yo + r, pcol = 8 * xo;
    const int base = prow * c.ES + pcol;
    uint32_t w[4];
    // branch-free: a dword outside the plane is read at offset 0 and replaced by zero, so the four loads (and those of the
    // caller's other segments) are in flight together -- as conditional loads each one was its own round trip
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const bool ok = prow < c.EH && pcol + 4 * d < c.ES;
        uint32_t v = *(const uint32_t*)(E + (ok ? base + 4 * d : 0));
        const int k = sc - (base + 4 * d);
        if (k >= 0 && k < 4) v = (v & ~(0xFFu << (8 * k))) | ((uint32_t)E_EMPTY << (8 * k));
        w[d] = ok ? v : 0u;
    }
    u32x4 out = {w[0], w[1], w[2], w[3]};
    return out;
}

// An env's C plane row (bbai_types.hpp) from its record by ONE wave: lane l = plane cell (l & 7, l >> 3); lanes < cpl_ids = the id bytes (an
// object stands on the grid iff the id plane holds it at its recorded position).  consume_env (reset()) and k_sync_cpl (imports).
__device__ __forceinline__ void cpl_build_wave(const LevelCfg& c, const uint8_t* __restrict__ rec, uint8_t* __restrict__ row, int lane) {
    const int x = lane & 7, y = lane >> 3;
    const int e = (x < c.W && y < c.H) ? (int)rec[e_index(c, x, y)] : (int)E_WALL;
    int v = 0xFF;
    if (lane < c.maxo) {
        const int ox = rec[c.off_pos + 2 * lane], oy = rec[c.off_pos + 2 * lane + 1];
        if (ox < c.W && oy < c.H && rec[c.off_I + i_index(c, ox, oy)] == lane + 2) v = oy << 3 | ox;
    }
    row[lane] = (uint8_t)e;
    if (lane < cpl_ids(c)) row[CPL_PLANE + lane] = (uint8_t)v;
}

// look-ahead slot -> live state of ONE env by ONE wave (k_consume: wave = env over the reset list; k_step<.., FUSE>: the wave that
// stepped the env): coalesced record copy, SoA verifier view, first observation of the new episode (to `obs_dst`: the caller's
// image row, or the block's LDS row in k_step), window plane + front cache, window bookkeeping for the batched refill.
// `win_meta` = the meta line of the tick's window (its M is raised when an env finishes for the second time inside one window).
// The job is a handful of kilobytes per env, so what it costs is its chain of dependent memory round trips (a reset-heavy small
// shard pays it on every step): everything that depends on nothing but the slot is LOADED FIRST, in batches that are all in
// flight together (pose, program, the record's 16-byte vectors, the window plane's row segments), the one load that needs the
// new pose (the view cell) goes out as soon as the pose is there, and the stores follow.  Round 3's form (load - store pairs
// in loops) was ten round trips long.
__device__ __forceinline__ void consume_env(const LevelCfg& c, int64_t n, int64_t env, int slot, int lane, uint8_t* recs,
                                            Hot* __restrict__ hots, uint64_t* __restrict__ stales, uint8_t* next_recs /* in-place: the start-carry patch goes into the slot */,
                                            const Hot* __restrict__ next_hots, uint32_t* __restrict__ vheads, uint64_t* __restrict__ vsets,
                                            int depth, uint8_t* __restrict__ pending, uint8_t* __restrict__ first_slot,
                                            uint32_t* __restrict__ win_meta, uint8_t* __restrict__ obs_dst, uint8_t* __restrict__ dirs,
                                            uint8_t* __restrict__ vplane /* or NULL */,
                                            uint16_t* __restrict__ fcache, uint8_t* __restrict__ lsm_arr /* or NULL */,
                                            bool inplace = false /* the slot BECOMES the live record: no copy; the slot the episode leaves is what gets refilled */,
                                            uint8_t* __restrict__ cplane = nullptr /* in-place small rooms: the env's C plane row is rebuilt from the slot */) {
    const int nvec = c.rec_bytes >> 4;
    uint8_t* nrec = next_recs + ring_at(slot, env, depth) * (int64_t)c.rec_bytes;
    Hot h = next_hots[ring_at(slot, env, depth)];
    const Prog* p = (const Prog*)(nrec + c.off_prog);
    const int start_carry = p->start_carry;
    const uint64_t pset = lane < 8 ? p->set[lane >> 1][lane & 1] : 0ull;
    const uint32_t vh = vhead_pack(*p);
    const int pend = lane == 0 ? (int)pending[env] : 0;
    h.slot = (uint8_t)(slot + 1 == depth ? 0 : slot + 1);
    // the view cell of the new pose (the one load that needs the pose)
    const int e_view = observe_fetch(c, nrec, h, lane);
    uint32_t fe0 = nrec[e_index(c, h.ax + dir_dx(h.dir), h.ay + dir_dy(h.dir))];       // (the front cell for the cache: with the view cells, not behind everything)
    // record: slot -> live copy
    if (!inplace) {
        const u32x4* src = (const u32x4*)nrec;
        u32x4* dst = (u32x4*)(recs + env * (int64_t)c.rec_bytes);
        constexpr int CPB = 2;
        for (int k0 = lane; k0 < nvec; k0 += 64 * CPB) {
            u32x4 buf[CPB];
#pragma unroll
            for (int j = 0; j < CPB; ++j) buf[j] = src[k0 + 64 * j < nvec ? k0 + 64 * j : nvec - 1];
            asm volatile("" : "+v"(buf[0]), "+v"(buf[1]));       // (both loads in flight before the first store: the scheduler otherwise pairs them load - store - load - store)
#pragma unroll
            for (int j = 0; j < CPB; ++j) if (k0 + 64 * j < nvec) dst[k0 + 64 * j] = buf[j];
        }
    }
    // the new episode's window plane, straight from the slot (L2 hits next to the copy above.  Parking the plane in LDS was
    // measured and dropped in round 3: any LDS at all makes k_consume's blocks queue behind the generator's waves for it)
    uint8_t* vrow = vplane ? vplane + env * (int64_t)v_bytes(c) : nullptr;
    if (vplane) {
        const int nseg = v_nxo(c) * v_nyo(c) * 8;
        constexpr int SGB = 4;
        for (int s0 = lane; s0 < nseg; s0 += 64 * SGB) {
            u32x4 seg[SGB];
#pragma unroll
            for (int j = 0; j < SGB; ++j) { const int sg = s0 + 64 * j < nseg ? s0 + 64 * j : nseg - 1; seg[j] = v_segment(c, nrec, sg >> 3, sg & 7, -1); }
#pragma unroll
            for (int j = 0; j < SGB; ++j) { const int sg = s0 + 64 * j; if (sg < nseg) *(u32x4*)(vrow + (sg >> 3) * VLINE + (sg & 7) * 16) = seg[j]; }
        }
    }
    uint8_t* crow = cplane ? cplane + env * (int64_t)cpl_bytes(c) : nullptr;
    if (crow) cpl_build_wave(c, nrec, crow, lane);
    // the verifier's SoA view of the new program
    if (lane < 8) vsets[(int64_t)lane * n + env] = pset;
    if (lane == 8) vheads[env] = vh;
    // first observation of the new episode, straight from the slot (identical bytes to the live copy)
    observe_emit(c, nrec, h, e_view, obs_dst, lane);
    if (lane == 0) {
        uint64_t stale0 = 0;
        uint32_t ce0 = E_EMPTY;
        // PutNext*Carrying: the first observation above still shows the object on the grid (the reference builds
        // it before handing the object to the agent, bonus_levels.py:821-829); now move it into the agent's hands.  In the
        // window plane (and the front cache) its cell is empty from the start.
        if (start_carry != NONE8) {
            const int sx = nrec[c.off_pos + 2 * start_carry], sy = nrec[c.off_pos + 2 * start_carry + 1];
            if (vplane) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the segment stores of every lane have landed; the patch goes over them
                v_patch(c, vrow, sx, sy, E_EMPTY);
            }
            if (crow) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the row bytes of the other lanes)
                crow[8 * sy + sx] = (uint8_t)E_EMPTY;
                crow[CPL_PLANE + start_carry] = 0xFF;
            }
            if (e_index(c, sx, sy) == e_index(c, h.ax + dir_dx(h.dir), h.ay + dir_dy(h.dir))) fe0 = E_EMPTY;
            ce0 = nrec[c.off_app + start_carry];
            apply_start_carry(c, inplace ? nrec : recs + env * (int64_t)c.rec_bytes, h, stale0, start_carry);
        }
        if (vplane || crow) fcache[env] = (uint16_t)(fe0 | (ce0 << 8));
        hots[env] = h;
        stales[env] = stale0;
        if (lsm_arr) lsm_arr[env] = 0;                  // fresh instruction objects: lastStepMatch = False (verifier.py:213-214)
        dirs[env] = h.dir;
        // window bookkeeping for the batched refill: first consumption in this window registers the env
        if (pend == 0) first_slot[env] = (uint8_t)(inplace ? live_slot(slot, depth) : slot);
        else atomicMax(win_meta, (uint32_t)(pend + 1));       // (rare: the env finished before in this window)
        pending[env] = (uint8_t)(pend + 1);
    }
}

// In-place layout: a finished env moves on to its next look-ahead slot, done by the env's OWN lane inside k_step (all the finished
// lanes of a wave side by side: no per-env loop, no tail).  Everything it needs depends on the slot alone -- pose, program, window
// bookkeeping and the new episode's first observation, which the generator wrote next to the level (computing it here, with the
// step's own window pipeline, doubled the vector work of every wave that carries a finished env: measured, profiles/r04/
// inplace_own_lane_observation_ab.jsonl) -- so it is ONE round trip, and it is issued the moment the lane knows its episode is over
// (advance_load, right behind the step's own stores); advance_finish swaps the SoA state of the env and puts the observation into
// the lane's LDS row.  Nothing here waits for another wave: the window keeps no list (see NWIN, bbai_kernels.hpp).
constexpr int OBS_BLOCK = 160;          // bytes of a next_obs slot that hold the first observation (147 used; sixteen-byte loads); OBS_SLOT / CPL_OFF: bbai_types.hpp
template <bool CP>
struct AdvanceRegs {
    u32x4 hv, tail /* Prog bytes 96..111: kind[4], root, n_a, n_b, strict, start_carry */, o[OBS_BLOCK / 16];
    u32x4 cp[CP ? (CPL_PLANE + CPL_MAX_IDS) / 16 : 1];      // the next level's C plane row
    uint64_t ps[8];
    uint32_t pend;
};
template <bool CP>
__device__ __forceinline__ void advance_load(const LevelCfg& c, int64_t env, int next /* hot.slot: the slot that becomes live */, int depth,
                                             const uint8_t* ring, const Hot* __restrict__ next_hots, const uint8_t* __restrict__ next_obs,
                                             const uint8_t* __restrict__ pending, AdvanceRegs<CP>& r) {
    const int64_t at = ring_at(next, env, depth);
    const uint8_t* nrec = ring + at * (int64_t)c.rec_bytes;
    r.hv = *(const u32x4*)(next_hots + at);
    const Prog* p = (const Prog*)(nrec + c.off_prog);
#pragma unroll
    for (int k = 0; k < 8; ++k) r.ps[k] = p->set[k >> 1][k & 1];
    r.tail = *(const u32x4*)((const uint8_t*)p + 96);
    r.pend = pending[env];
    const u32x4* ob = (const u32x4*)(next_obs + at * OBS_SLOT);
#pragma unroll
    for (int k = 0; k < OBS_BLOCK / 16; ++k) r.o[k] = ob[k];
    if constexpr (CP) {
        const u32x4* cr = (const u32x4*)(next_obs + at * OBS_SLOT + CPL_OFF);
#pragma unroll
        for (int k = 0; k < (CPL_PLANE + CPL_MAX_IDS) / 16; ++k) r.cp[k] = cr[k];      // (the slot holds 96 bytes whatever the level's id count)
    }
}
template <bool CP>
__device__ __forceinline__ void advance_finish(const LevelCfg& c, int64_t n, int64_t env, int lane, int next, int depth, uint8_t* ring, const AdvanceRegs<CP>& r,
                                               Hot* __restrict__ hots, uint64_t* __restrict__ stales, uint32_t* __restrict__ vheads, uint64_t* __restrict__ vsets,
                                               uint8_t* __restrict__ pending, uint8_t* __restrict__ first_slot, uint32_t* __restrict__ win_meta,
                                               uint8_t* __restrict__ s_rows, uint8_t* __restrict__ dirs, uint8_t* __restrict__ lsm_arr,
                                               uint8_t* __restrict__ cplane, uint16_t* __restrict__ fcache) {
    static_assert(sizeof(Prog) == 112 && offsetof(Prog, kind) == 96 && offsetof(Prog, start_carry) == 104, "Prog tail");
    Hot h;
    __builtin_memcpy(&h, &r.hv, sizeof(h));
    h.slot = (uint8_t)(next + 1 == depth ? 0 : next + 1);
    Prog pt;                                    // (only the tail fields are read below)
    __builtin_memcpy((uint8_t*)&pt + 96, &r.tail, 16);
    const uint32_t vh = vhead_pack(pt);
    const int start_carry = pt.start_carry;
    {
        RowPacker rp(s_rows, lane);
#pragma unroll
        for (int j = 0; j < 37; ++j) rp.put(j, r.o[j >> 2][j & 3]);
        rp.finish();
    }
    uint64_t stale0 = 0;
    uint32_t ce0 = E_EMPTY;
    if constexpr (CP) {
        u32x4* crow = (u32x4*)(cplane + env * (int64_t)cpl_bytes(c));
        const int nv = cpl_bytes(c) >> 4;
#pragma unroll
        for (int k = 0; k < (CPL_PLANE + CPL_MAX_IDS) / 16; ++k) if (k < nv) crow[k] = r.cp[k];
    }
    // PutNext*Carrying (consume_env): the first observation shows the object on the grid; now it is in the agent's hands
    if (start_carry != NONE8) {
        uint8_t* nrec = ring + ring_at(next, env, depth) * (int64_t)c.rec_bytes;
        if constexpr (CP) {
            const int sx = nrec[c.off_pos + 2 * start_carry], sy = nrec[c.off_pos + 2 * start_carry + 1];
            ce0 = nrec[c.off_app + start_carry];
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the row above has landed; the patch goes over it
            uint8_t* crow = cplane + env * (int64_t)cpl_bytes(c);
            crow[8 * sy + sx] = (uint8_t)E_EMPTY;
            crow[CPL_PLANE + start_carry] = 0xFF;
        }
        apply_start_carry(c, nrec, h, stale0, start_carry);
    }
    if constexpr (CP) fcache[env] = (uint16_t)(E_EMPTY | (ce0 << 8));
#pragma unroll
    for (int k = 0; k < 8; ++k) vsets[(int64_t)k * n + env] = r.ps[k];
    vheads[env] = vh;
    hots[env] = h;
    stales[env] = stale0;
    if (lsm_arr) lsm_arr[env] = 0;
    dirs[env] = h.dir;
    if (r.pend == 0) first_slot[env] = (uint8_t)live_slot(next, depth);      // the slot this env's finished episode lived in: free for the refill
    else atomicMax(win_meta, r.pend + 1u);
    pending[env] = (uint8_t)(r.pend + 1);
}

// VP: the window comes from the env's V-plane line (ONE 128-byte line per step) and the transition's inputs -- the
// appearance of the front cell and of the carried object -- from the 2-byte cache the previous step left (`fcache`), so a
// plain move / turn touches no other record line; without VP both come out of the record (round 2's path: 2-3 lines for
// the window + the lines of the front cell's id and the carried object's appearance).
// FUSE: a wave whose envs finished consumes their look-ahead slots ITSELF (consume_env for every set bit of the wave's ballot,
// the new episode's first observation straight into the block's LDS rows), instead of listing them for a k_consume launch.
// `fuse` carries what k_consume's arguments carried.
// The step's own tap (bbai_step_tapped): the listed envs' outputs of THIS step into caller-owned log rows, written by the stepping lanes
// themselves -- what a bbai_tap_ids launch behind the step would copy, without the launch (k_tap is 3 us + a dependent-launch gap: a quarter
// of a 65 536-env step).  mask[block] bit l = env 64 block + l is listed; its log row = perm[rank0[block] + listed envs below it in the block].
struct TapArgs {
    const unsigned long long* mask; const uint32_t* rank0; const int32_t* perm;
    uint8_t* image_out; uint8_t* dir_out; double* rew_out; uint8_t* done_out;
    int64_t count;        // listed envs = log rows per tick (a launch of several ticks moves on by one row set per tick)
};
struct FuseArgs {
    uint8_t* next_recs; const Hot* next_hots; const uint8_t* next_obs; int depth;
    uint8_t* pending; uint8_t* first_slot; uint32_t* win_meta; unsigned long long* totals;
};
// step_body: ONE tick of a 64-env block (the whole of k_step; k_step_ticks calls it once per tick).  `s_obs`: the block's LDS rows.
// The hold action (option "step_hold", include/bbai.h BBAI_ACTION_HOLD): `hold` = the action byte that means "this env sits this step out", or -1
// (the option is off, or the actions are the expert's) -- then no byte compares equal and nothing below differs from a build without it.
//   a held lane in a wave that steps   takes the frozen arm: its row goes through LDS unchanged (CP: the deferred copy behind the wave barrier), it stores
//                                      nothing else -- no state, no reward / done / direction, no lastStepMatch byte -- and never asks for a reset, not even
//                                      as an env the generator gave up on (frozen == 2: that skip waits for the env's next real step);
//   a wave in which nobody steps       leaves behind its one coalesced action load -- false is returned: no SoA state, no plane or record line, no LDS row,
//                                      no store loop over the block's span, no counter.  One wave is one block: the branch is uniform, and the barriers
//                                      further down are reached by all of a block or by none.  A wave with a listed env of the step's own tap stays: a held,
//                                      listed env logs its unchanged outputs (one row per listed env per step).
template <bool VP, int FUSE /* 0: finished envs listed for k_consume; 1: consumed by the stepping wave (consume_env); 3: in-place layout (advance_load / advance_finish) */,
          bool CP = false /* in-place small single rooms: pose-independent C plane row instead of the record's planes (bbai_types.hpp) */>
__device__ __forceinline__ bool step_body(const LevelCfg& c, int64_t n, uint8_t* __restrict__ recs,
                                                     Hot* __restrict__ hots, uint64_t* __restrict__ stales,
                                                     uint32_t* vheads, uint64_t* vsets /* read by every lane, WRITTEN for the envs the wave moves on (FUSE): no restrict */,
                                                     const uint8_t* __restrict__ actions, uint8_t* image /* read (frozen envs re-emit) AND written: no restrict */,
                                                     uint8_t* __restrict__ dirs, float* __restrict__ rewards,
                                                     double* __restrict__ rewards64, uint8_t* __restrict__ dones, int auto_reset,
                                                     int32_t* __restrict__ reset_list, uint8_t* __restrict__ reset_slot, uint32_t* __restrict__ counters,
                                                     int prio, uint8_t* __restrict__ vplane, uint16_t* __restrict__ fcache,
                                                     uint8_t* __restrict__ lsm_arr /* NULL, or the done-action mode's per-env bits */,
                                                     int enum_done /* done-action mode: this step's `done` actions are the enum member (bbai_step.hpp verify_side) */,
                                                     int hold /* the action byte of an env that sits this step out (A_HOLD), or -1: none does */,
                                                     FuseArgs fuse, int64_t block0 /* first 64-env block of this launch (bbai_step_render steps the batch in two halves) */,
                                                     uint8_t* __restrict__ cplane /* CP: [n][cpl_bytes] */, const TapArgs& tap /* mask == NULL: none */,
                                                     uint8_t* const s_obs, const int lane /* threadIdx.x */, const int blk_x /* blockIdx.x */) {
    static_assert(!CP || (FUSE == 3 && !VP), "the C plane belongs to the in-place layout");
    uint8_t* const s_rows = s_obs + ROWS_FRONT;
    if (prio) __builtin_amdgcn_s_setprio(3);            // the look-ahead generator's waves share the CUs: issue ours first
    const int64_t env0 = ((int64_t)blk_x + block0) * STEP_BLOCK;
    const int64_t env = env0 + lane;
    const bool active = env < n;
    int action = 0;
    if (hold >= 0) {
        // the hold action is on: the wave's actions come first, on their own (one more round trip in front of a wave that steps, the price of a
        // wave that does not step costing one 64-byte load), and a wave none of whose envs steps is done
        action = active ? (int)actions[env] : hold;
        const bool listed = tap.mask && tap.mask[(int64_t)blk_x + block0] != 0;
        if (!listed && !__ballot(action != hold)) return false;
    }
    bool want_reset = false;
    bool frozen_copy = false; // CP: a frozen lane's row copy, deferred until every lane has read its parked plane (below)
    int my_slot = 0;
    AdvanceRegs<CP> adv;      // (in-place layout: the finished lanes' next-slot loads)
    if (active) {
        // everything the step needs from the SoA arrays in ONE memory round trip, before the frozen test (the loads the
        // branch would otherwise delay are a second round trip on every step's critical path)
        u32x4 hv = *(const u32x4*)(hots + env);
        uint64_t stale = stales[env];
        VProg vp; vp.bind(vheads[env], vsets + env, n);
        if (hold < 0) action = actions[env];
        uint32_t fc = (VP || CP) ? (uint32_t)fcache[env] : 0u;
        Lsm lsm = {lsm_arr ? (uint32_t)lsm_arr[env] : 0u, lsm_arr != nullptr};
        // CP: the env's whole grid + object positions come with the SoA state -- nothing below depends on a second memory round trip
        u32x4 pv[4] = {}, iv[2] = {};
        uint8_t* crow = nullptr;
        if constexpr (CP) {
            crow = cplane + env * (int64_t)cpl_bytes(c);
            const u32x4* cr = (const u32x4*)crow;
#pragma unroll
            for (int k = 0; k < 4; ++k) pv[k] = cr[k];
            iv[0] = cr[4];
            const u32x4 none = {~0u, ~0u, ~0u, ~0u};
            iv[1] = none;
            if (cpl_ids(c) > 16) iv[1] = cr[5];
            asm volatile("" : "+v"(pv[0]), "+v"(pv[1]), "+v"(pv[2]), "+v"(pv[3]), "+v"(iv[0]), "+v"(iv[1]));
        }
        // (the empty asm pins the loaded values here: the compiler would otherwise sink the loads into the branch)
        asm volatile("" : "+v"(hv), "+v"(stale), "+v"(vp.head), "+v"(vp.set00), "+v"(action), "+v"(fc));
        Hot h;
        __builtin_memcpy(&h, &hv, sizeof(h));
        my_slot = h.slot;
        uint8_t* rec = FUSE == 3 ? fuse.next_recs + ring_at(live_slot(h.slot, fuse.depth), env, fuse.depth) * (int64_t)c.rec_bytes : recs + env * (int64_t)c.rec_bytes;
        const bool held = action == hold;      // (never with hold = -1: a byte is 0..255)
        if (!h.frozen && !held) {
            double reward = 0.0;
            const EnvRef r = env_ref(c, rec, vp);
            uint8_t* vrow = VP ? vplane + env * (int64_t)v_bytes(c) : nullptr;
            int fe, ce;
            // CP: the lane's plane parked in LDS (8 rows x 8 bytes at a 72-byte lane pitch, inside the block's obs-row area: every lane's reads of
            // it precede, in the one wave's program order, every lane's row writes at the end of the step), for the per-lane row / cell addressing
            uint8_t* const pl = s_obs + lane * 72;
            if constexpr (CP) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    *(uint2*)(pl + 16 * k) = make_uint2(pv[k][0], pv[k][1]);
                    *(uint2*)(pl + 16 * k + 8) = make_uint2(pv[k][2], pv[k][3]);
                }
                fe = pl[8 * (h.ay + dir_dy(h.dir)) + h.ax + dir_dx(h.dir)];
                ce = (int)(fc >> 8);
            } else if (VP) {
                fe = (int)(fc & 0xFFu); ce = (int)(fc >> 8);
            } else {
                fe = r.E[e_index(c, h.ax + dir_dx(h.dir), h.ay + dir_dy(h.dir))];
                ce = h.carry != NONE8 ? r.app[h.carry] : (int)E_EMPTY;
            }
            if (action != A_RESET_ENV) apply_pose(h, action, fe);
            // the 7x7 window of the pose after the action.  Grid.slice extents (get_view_exts): its top-left world cell
            const int dir = h.dir;
            const int txm = h.ax + MARGIN + (dir == 0 ? 0 : dir == 2 ? -6 : -3);
            const int tym = h.ay + MARGIN + (dir == 1 ? 0 : dir == 3 ? -6 : -3);
            uint32_t wd[3 * VIEW];
            uint32_t wl[VIEW], wh[VIEW];
            if constexpr (CP) {
                window_rows_cpl(pl, c.H, h.ax, h.ay, dir, wl, wh);
            } else if (VP) {
                const uint8_t* line = vrow + ((tym >> 1) * v_nxo(c) + (txm >> 3)) * VLINE + (tym & 1) * 16 + (txm & 4);
                window_fetch((const uint32_t*)line, 4, wd);
            } else {
                window_fetch((const uint32_t*)(rec + ((tym * c.ES + txm) & ~3)), c.ES >> 2, wd);     // (ES is a multiple of 4)
            }
            // the id-plane entry of the front cell, fetched WITH the window: the verifier's common question ("is the object
            // in front of me one of the described ones") and the object actions then need no further memory round trip
            // (BBAI_PREFETCH_ID=0: read lazily, as rounds 1-2 did -- one more line per env-step, one round trip less)
            int idf = -1;
#if BBAI_PREFETCH_ID
            idf = r.I[i_index(c, h.ax + dir_dx(dir), h.ay + dir_dy(dir))];
#endif
            const int fpos = (h.ay + dir_dy(dir)) << 3 | (h.ax + dir_dx(dir));      // CP: the front cell in C plane coordinates
            if constexpr (CP) {
                const uint32_t idw[8] = {iv[0][0], iv[0][1], iv[0][2], iv[0][3], iv[1][0], iv[1][1], iv[1][2], iv[1][3]};
                idf = cid_lookup(idw, 8, fpos);                 // (what r.I would say about an object there; 0 = none)
            }
            // pickup / drop / toggle, while the window is on its way
            int nfe = -1;
            if (action != A_RESET_ENV) {
                int nid = -1;
                nfe = apply_objects(c, r, h, stale, action, fe, ce, idf, &nid);
                if (VP && nfe >= 0) v_patch(c, vrow, h.ax + dir_dx(dir), h.ay + dir_dy(dir), nfe);
                if constexpr (CP) {          // the env's C plane row follows the record: the cell, and who stands (or no longer stands) on it
                    if (nfe >= 0) crow[fpos] = (uint8_t)nfe;
                    if (nid >= 0) {
                        if (idf >= 2) crow[CPL_PLANE + idf - 2] = 0xFF;              // picked up / an opened box
                        if (nid >= 2) crow[CPL_PLANE + nid - 2] = (uint8_t)fpos;     // dropped / a box's content
                    }
                }
                if (idf >= 0 && nid >= 0) idf = nid;
            }
            int fe2;
            uint32_t cp[13];
#if BBAI_VIEW_LDS
            uint32_t vis[VIEW];
            view_cells(wd, txm & 3, dir, (uint32_t)ce, nfe, s_rows + row_scratch(lane), cp, vis, fe2);
#else
            if constexpr (CP) view_rows_perm(wl, wh, dir, (uint32_t)ce, nfe, cp, fe2);
            else view_cells_perm(wd, txm & 3, dir, (uint32_t)ce, nfe, cp, fe2);       // (bbai_view.hpp: rotation, occlusion and masking in registers)
#endif
            // "env.reset() for THIS env, now" (A_RESET_ENV, bbai_step.hpp): the episode ends with done = 1, reward = 0
            const bool done = action == A_RESET_ENV ? true : finish_step(c, r, h, stale, action, fe2, reward, lsm, idf, enum_done != 0);
            if (lsm_arr) lsm_arr[env] = (uint8_t)lsm.bits;
            if (done && !auto_reset) h.frozen = 1;
            want_reset = done && auto_reset;
            hots[env] = h;
            stales[env] = stale;
            if (VP || CP) fcache[env] = (uint16_t)((uint32_t)fe2 | ((uint32_t)ce << 8));
            rewards[env] = (float)reward;
            if (rewards64) rewards64[env] = reward;        // the reference's Python float, bit for bit (levelgen.py:59-61)
            dones[env] = done ? 1 : 0;
            dirs[env] = h.dir;
#if BBAI_VIEW_LDS
            encode_view(cp, vis, RowPacker(s_rows, lane));
#else
            encode_cells(cp, RowPacker(s_rows, lane));
#endif
        }
        // frozen envs keep re-emitting their last outputs: copy them through LDS unchanged; so does an env that holds
        else {
            if (h.frozen == 2 && auto_reset && !held) {      // level the generator gave up on (last-resort guard): skip to the next one
                rewards[env] = 0.0f;
                if (rewards64) rewards64[env] = 0.0;
                dones[env] = 1;
                want_reset = true;
            }
            if constexpr (CP) {
                frozen_copy = true;
            } else {
                const uint8_t* src = image + env * OBS_BYTES;
                for (int b = 0; b < OBS_BYTES; ++b) s_rows[lane * OBS_BYTES + b] = src[b];
            }
        }
        if constexpr (FUSE == 3) { if (want_reset) advance_load<CP>(c, env, my_slot, fuse.depth, fuse.next_recs, fuse.next_hots, fuse.next_obs, fuse.pending, adv); }
    }
    if constexpr (CP) {
        // The stepping lanes parked their planes INSIDE the obs-row area (at a 72-byte pitch: over other lanes' rows).  Their own rows are written
        // after every plane read by the wave's program order; a frozen lane's row copy sits in the other arm of a branch, which the compiler may
        // emit FIRST -- the parked planes then went over rows already copied (caught by test_manyenvs_freeze).  So it waits here, behind a
        // convergent fence that no arm of that branch can cross.
        __builtin_amdgcn_wave_barrier();
        if (frozen_copy) {
            const uint8_t* src = image + env * OBS_BYTES;
            for (int b = 0; b < OBS_BYTES; ++b) s_rows[lane * OBS_BYTES + b] = src[b];
        }
    }
    // finished envs.  Unfused: compacted into the reset list for k_consume (one returning atomic per wave).  Fused / in-place: counted
    // (one fire-and-forget add to this block's shard of the total) and moved on by this wave itself.
    {
        unsigned long long bal = __ballot(want_reset);
        if (bal) {
            const int leader = __ffsll((long long)bal) - 1;
            if constexpr (FUSE == 0) {
                uint32_t basei = 0;
                if (lane == leader) basei = atomicAdd(&counters[0], (uint32_t)__popcll(bal));
                basei = __shfl(basei, leader);
                if (want_reset) {
                    const uint32_t at = basei + __popcll(bal & ((1ull << lane) - 1));
                    reset_list[at] = (int32_t)env;
                    reset_slot[at] = (uint8_t)my_slot;
                }
            } else if constexpr (FUSE == 3) {
                // in-place layout: every finished lane moves its own env on (its stores to its own SoA entries stay in program order)
                if (lane == leader) count_resets(fuse.totals, (unsigned int)__popcll(bal), (unsigned int)blk_x);
                if (want_reset)
                    advance_finish<CP>(c, n, env, lane, my_slot, fuse.depth, fuse.next_recs, adv, hots, stales, vheads, vsets, fuse.pending, fuse.first_slot,
                                       fuse.win_meta, s_rows, dirs, lsm_arr, cplane, fcache);
            } else {
                // Everything this wave stored to the records, window planes and SoA entries of these envs must have landed
                // before other lanes overwrite them (a terminal pickup patches the record the consume is about to replace).
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane == leader) count_resets(fuse.totals, (unsigned int)__popcll(bal), (unsigned int)blk_x);
                while (bal) {
                    const int src = __ffsll((long long)bal) - 1;
                    bal &= bal - 1;
                    const int slot = __shfl(my_slot, src);
                    // (the new episode's first observation goes over the finished env's row; LDS traffic of the one wave stays in program order)
                    consume_env(c, n, env0 + src, slot, lane, recs, hots, stales, fuse.next_recs, fuse.next_hots, vheads, vsets,
                                fuse.depth, fuse.pending, fuse.first_slot, fuse.win_meta, s_rows + src * OBS_BYTES, dirs,
                                VP ? vplane : nullptr, fcache, lsm_arr);
                }
            }
        }
    }
    __syncthreads();
    // the block's contiguous obs span leaves as it lies in LDS: 16 bytes per lane per store (64 x 147 B = 588 x 16 B; the
    // span of every full block starts 16-byte aligned in the output).  The last, partial block ends with a byte tail.
    const int64_t nb = n - env0 < STEP_BLOCK ? n - env0 : STEP_BLOCK;      // envs in this block
    const int total = (int)nb * OBS_BYTES;
    uint8_t* out = image + env0 * OBS_BYTES;
    {
        // (a caller's buffer that is not 16-byte aligned -- a row of a [T][n][147] history with odd n -- gets dwords or bytes)
        const int al = (int)((uintptr_t)out & 15);
        int done_bytes = 0;
        if (al == 0) {
            const int nvec = total >> 4;
            const u32x4* s128 = (const u32x4*)s_rows;
            for (int v = lane; v < nvec; v += STEP_BLOCK) ((u32x4*)out)[v] = s128[v];     // (non-temporal here: measured, no effect -- profiles/r03/NOTES.md)
            done_bytes = nvec << 4;
        } else if ((al & 3) == 0) {
            const int ndw = total >> 2;
            const uint32_t* s32 = (const uint32_t*)s_rows;
            for (int d = lane; d < ndw; d += STEP_BLOCK) ((uint32_t*)out)[d] = s32[d];
            done_bytes = ndw << 2;
        }
        for (int b = done_bytes + lane; b < total; b += STEP_BLOCK) out[b] = s_rows[b];
    }
    // the step's own tap: a listed env's row out of LDS (for an env that finished: already its new episode's first observation), its direction /
    // reward / done as this wave stored them (agent-scope loads: the direction of a consumed env was stored by another lane)
    if (tap.mask) {
        const int64_t blk = (int64_t)blk_x + block0;
        const unsigned long long tm = tap.mask[blk];
        if (active && (tm >> lane & 1ull)) {
            const int64_t row = (int64_t)tap.perm[tap.rank0[blk] + (uint32_t)__popcll(tm & ((1ull << lane) - 1ull))];
            uint8_t* o = tap.image_out + row * OBS_BYTES;
            const uint8_t* srow = s_rows + lane * OBS_BYTES;
            for (int b = 0; b < OBS_BYTES; ++b) o[b] = srow[b];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            tap.dir_out[row] = __hip_atomic_load(dirs + env, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            tap.done_out[row] = __hip_atomic_load(dones + env, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            tap.rew_out[row] = __hip_atomic_load(rewards64 + env, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    return true;
}
// The dirty cells of a step whose render is a delta render of the registered target (render_launch: k_render_dstore).  k_step's tail, after
// step_body has stored the block's rows: lanes over (env, cell) of the block's 64 rows, 16 cells per lane and chunk -- the chunk's 16 shadow
// bytes in one coalesced 16-byte load, its 48 encoding bytes in three 16-byte LDS reads (a row is 49 cells at the output pitch of 147 =
// 3 x 49: cell b of the block is LDS bytes [3 b, 3 b + 3)) -- the new tile id of every cell (the same s_lut lookup as k_render, the agent's
// table for AGENT_CELL; four cells per word, dirty_chunk of bbai_dirty.hpp), the changed ones written back to the shadow (the chunk whole,
// where one differs), and per env a 64-bit dirty mask (bit = cell) into `dmask`: the chunk's 16 changed-cell bits split at the env boundary
// (dirty_split) and gathered by LDS atomics in the first 512 bytes of the row area, which nothing reads any more.
constexpr int DIRTY_CHUNKS = (STEP_BLOCK * CELLS / 16 + STEP_BLOCK - 1) / STEP_BLOCK;      // 16-byte shadow chunks per lane: 196 per block -> 4
static_assert(STEP_BLOCK * CELLS % 16 == 0 && OBS_BYTES == 3 * CELLS, "a block's shadow rows are whole 16-byte chunks; a row is 3 bytes per cell");
static_assert(DIRTY_CELLS == CELLS && DIRTY_AGENT == AGENT_CELL && DIRTY_CHUNK == 16, "bbai_dirty.hpp restates the view's geometry for the host build");
__device__ __forceinline__ void step_dirty(int64_t n, int64_t env0, uint8_t* __restrict__ shadow /* [n][49] */, uint64_t* __restrict__ dmask /* [n] */,
                                           const uint8_t* __restrict__ lut, uint8_t* const s_rows, uint8_t* const s_lut, const int lane) {
    const int nb = n - env0 < STEP_BLOCK ? (int)(n - env0) : STEP_BLOCK;
    const int nbytes = nb * CELLS;
    uint8_t* const sh = shadow + env0 * CELLS;                   // (16-byte aligned: env0 is a multiple of 64)
    const uint2 lv = ((const uint2*)lut)[lane];
    uint32_t old[DIRTY_CHUNKS][4];
#pragma unroll
    for (int k = 0; k < DIRTY_CHUNKS; ++k) {
        const int v = lane + k * STEP_BLOCK;
        old[k][0] = old[k][1] = old[k][2] = old[k][3] = 0;
        if (16 * v + 16 <= nbytes) {
            const u32x4 w = ((const u32x4*)sh)[v];
            old[k][0] = w[0]; old[k][1] = w[1]; old[k][2] = w[2]; old[k][3] = w[3];
        } else {                                                 // (the last, partial block's last chunk)
            for (int i = 0; i < 16 && 16 * v + i < nbytes; ++i) old[k][i >> 2] |= (uint32_t)sh[16 * v + i] << (8 * (i & 3));
        }
    }
    *(uint2*)(s_lut + 8 * lane) = lv;
    __syncthreads();                                             // (one wave: the lut's LDS writes before its reads)
    uint64_t ma[DIRTY_CHUNKS], mb[DIRTY_CHUNKS];                 // the chunk's dirty cells in its first env, and in the next one
#pragma unroll
    for (int k = 0; k < DIRTY_CHUNKS; ++k) {
        const int v = lane + k * STEP_BLOCK;
        ma[k] = mb[k] = 0;
        if (16 * v >= nbytes) continue;
        const u32x4* enc = (const u32x4*)(s_rows + 48 * v);
        const u32x4 q0 = enc[0], q1 = enc[1], q2 = enc[2];
        const uint32_t ew[12] = {q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3], q2[0], q2[1], q2[2], q2[3]};
        // four cells per word (bbai_dirty.hpp): keys by byte permutes, the agent's id patched in once per chunk, the changed cells as 16 bits
        const int c0 = 16 * v - 16 * v / CELLS * CELLS;          // the chunk's first cell
        uint32_t nw[4];
        const uint32_t bits = dirty_chunk(ew, old[k], s_lut, c0, nbytes - 16 * v, nw);
        dirty_split(bits, c0, ma[k], mb[k]);
        if (bits) {
            if (16 * v + 16 <= nbytes) { u32x4 w = {nw[0], nw[1], nw[2], nw[3]}; ((u32x4*)sh)[v] = w; }
            else for (int i = 0; i < 16 && 16 * v + i < nbytes; ++i) sh[16 * v + i] = (uint8_t)(nw[i >> 2] >> (8 * (i & 3)));
        }
    }
    __syncthreads();                                             // every lane has read its rows: their first 512 bytes take the masks
    unsigned long long* const s_dm = (unsigned long long*)s_rows;
    s_dm[lane] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < DIRTY_CHUNKS; ++k) {
        const int ea = 16 * (lane + k * STEP_BLOCK) / CELLS;
        if (ma[k]) atomicOr(s_dm + ea, (unsigned long long)ma[k]);
        if (mb[k]) atomicOr(s_dm + ea + 1, (unsigned long long)mb[k]);
    }
    __syncthreads();
    if (lane < nb) dmask[env0 + lane] = s_dm[lane];
}

// What a step launch is given: the kernels' one argument (the kernarg segment IS this struct).
struct StepArgs {
    LevelCfg c; int64_t n; uint8_t* recs; Hot* hots; uint64_t* stales; uint32_t* vheads; uint64_t* vsets; const uint8_t* actions; uint8_t* image; uint8_t* dirs;
    float* rewards; double* rewards64; uint8_t* dones; int auto_reset; int32_t* reset_list; uint8_t* reset_slot; uint32_t* counters; int prio; uint8_t* vplane;
    uint16_t* fcache; uint8_t* lsm_arr; int enum_done; int hold /* step_body: the hold action's byte, or -1 */; FuseArgs fuse; int64_t block0; uint8_t* cplane; TapArgs tap;
    int ticks;            // k_step_ticks: steps this launch takes; tick t reads actions + t n and logs into the tap rows t * tap.count further on
    uint8_t* dshadow; uint64_t* dmask; const uint8_t* lut;     // k_step: dshadow != NULL = the dirty cells of this step for its delta render (step_dirty)
};
template <bool VP, int FUSE, bool CP = false>
__global__ __launch_bounds__(STEP_BLOCK, BBAI_STEP_WAVES) void k_step(StepArgs a) {
    // the block's observation rows at the OUTPUT pitch of 147 bytes (bbai_step.hpp RowPacker), 16 bytes of front padding
    __shared__ __attribute__((aligned(16))) uint8_t s_obs[ROWS_FRONT + STEP_BLOCK * OBS_BYTES + 16];
    __shared__ __attribute__((aligned(8))) uint8_t s_lut[512];      // step_dirty (9 952 bytes in all: 16 blocks = 16 waves still fit a CU's 160 KiB)
    const bool stepped = step_body<VP, FUSE, CP>(a.c, a.n, a.recs, a.hots, a.stales, a.vheads, a.vsets, a.actions, a.image, a.dirs, a.rewards, a.rewards64, a.dones, a.auto_reset,
                            a.reset_list, a.reset_slot, a.counters, a.prio, a.vplane, a.fcache, a.lsm_arr, a.enum_done, a.hold, a.fuse, a.block0, a.cplane, a.tap, s_obs, (int)threadIdx.x,
                            (int)blockIdx.x);
    if (!stepped) {
        // every env of the wave held: none of their cells is dirty -- said here, or the store-only render would store last step's pieces again
        const int64_t env = ((int64_t)blockIdx.x + a.block0) * STEP_BLOCK + threadIdx.x;
        if (a.dshadow && env < a.n) a.dmask[env] = 0;
        return;
    }
    if (a.dshadow) step_dirty(a.n, ((int64_t)blockIdx.x + a.block0) * STEP_BLOCK, a.dshadow, a.dmask, a.lut, s_obs + ROWS_FRONT, s_lut, (int)threadIdx.x);
}
// Several ticks in one launch (bbai_rollout, open-loop actions): an env's step touches only its own state, its block's LDS rows and -- for a
// finished env -- look-ahead slots the window gate in front of the launch has vouched for, so a block walks through its ticks on its own, with
// no launch boundary (and no dependent-launch gap: 4-5 us, a third of a 65 536-env step) in between.  Everything a tick reads of the previous one
// was stored by THIS wave: its vector-memory operations stay in program order.
// Every tick reads its arguments from the kernarg segment AGAIN, through a pointer the compiler cannot see through: left to itself it hoists
// what the ticks share (fifty LevelCfg words, thirty pointers and all that derives from them) out of the loop and keeps it in registers across
// the body -- 251 VGPRs against 93, two waves per SIMD against five.
typedef const StepArgs __attribute__((address_space(4))) * StepArgsPtr;
// ... and the register budget is the four waves per SIMD the one-tick kernels of the default paths have (115-117 VGPRs): the constants the
// loop optimiser still parks in registers in front of the loop are rematerialised or, a handful, spilled (2-7 VGPRs: kernel_resources.json).
template <bool VP, int FUSE, bool CP = false>
__global__ __launch_bounds__(STEP_BLOCK, 4) void k_step_ticks(StepArgs a_) {
    __shared__ __attribute__((aligned(16))) uint8_t s_obs[ROWS_FRONT + STEP_BLOCK * OBS_BYTES + 16];
    const int ticks = a_.ticks;
    for (int tick = 0; tick < ticks; ++tick) {
        StepArgsPtr ap = (StepArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
        int t = tick, lane = (int)threadIdx.x, blk_x = (int)blockIdx.x;        // (the lane and block arithmetic likewise: re-derived per tick)
        asm volatile("" : "+s"(ap), "+s"(t), "+v"(lane), "+s"(blk_x));
        const StepArgs a = *(const StepArgs*)ap;          // (InferAddressSpaces turns these back into scalar loads of the constant segment)
        TapArgs tap = a.tap;
        tap.image_out += (int64_t)t * tap.count * OBS_BYTES; tap.dir_out += (int64_t)t * tap.count; tap.rew_out += (int64_t)t * tap.count; tap.done_out += (int64_t)t * tap.count;
        // (a tick in which the whole wave holds -- step_body returns false behind its action load -- is just the next tick)
        step_body<VP, FUSE, CP>(a.c, a.n, a.recs, a.hots, a.stales, a.vheads, a.vsets, a.actions + (int64_t)t * a.n, a.image, a.dirs, a.rewards, a.rewards64, a.dones, a.auto_reset,
                                a.reset_list, a.reset_slot, a.counters, a.prio, a.vplane, a.fcache, a.lsm_arr, a.enum_done, a.hold, a.fuse, a.block0, a.cplane, tap, s_obs, lane, blk_x);
        __syncthreads();        // (one wave per block: orders this tick's LDS reads before the next one's writes for the compiler)
    }
}
