// ------------------------------------------------------------------------------------------
// Demonstrations that stay on the device (babyai_amd/imitation.py DemoStore / DemoBatch):
//   k_demo_spans  one chunk of bbai_bot_rollout history -> every stream's first solved episode (demos.py scan_chunk)
//   k_demo_pack   the spans of up to C history chunks   -> the store's flat arrays
//   k_demo_batch  a sorted list of demos of a store     -> the flat batch of imitation.py:226-251 (or a sub-store)
//   k_demo_jobs   one chunk of history of a POOL of envs that play listed seeds (DemoStore.collect_seeds) -> the episodes that ended,
//                 kept or dropped, and the next seed of every env that finished
//   k_demo_pack_list  k_demo_pack for a list of (stream, first step, length) records in a ring of history chunks
//   k_demo_replay_feed / k_demo_replay_judge  a POOL of envs that plays a store's demonstrations back (DemoStore.replay):
//                 before the step, compare every playing env's observation with the recorded frame and hand out the recorded action;
//                 behind it, score the envs that were fed and give the free ones the next demos
// The two copies write ALIGNED 16-byte chunks of one contiguous destination; a chunk's bytes come from at most two source
// runs (147-byte history rows in k_demo_pack, whole demos in k_demo_batch), each fetched as two aligned 16-byte loads
// and byte-aligned in registers.  Every unaligned 16-byte window that is fetched lies INSIDE a source run (a chunk that
// crosses into the next run takes the run's last 16 bytes and the next run's first 16, and shifts the pair), so the
// aligned loads around it stay inside any allocation that starts 16-byte aligned and is a multiple of 16 bytes long.
// ------------------------------------------------------------------------------------------
#pragma once
#include <hip/hip_runtime.h>
#include "bbai_kernels.hpp"      // u32x4

namespace bbai {

constexpr int DEMO_BLOCK = 256;                 // lanes per block
constexpr int DEMO_UNROLL = 2;                  // 16-byte chunks per lane: both chunks' loads are issued before the first store
constexpr int DEMO_BLOCK_BYTES = DEMO_BLOCK * DEMO_UNROLL * 16;
constexpr int DEMO_SLICE = 64;                  // runs a block can meet: 8192 / 147 + 2 = 57 frames, every demo holds at least one
constexpr uint32_t DEMO_ROW = 147;              // bytes of one 7x7x3 frame
constexpr uint32_t DEMO_DIV147 = 29217465u;     // ceil(2^32 / 147): __umulhi(x, .) == x / 147 for x < 7 * 10^7

struct DemoChunkPtrs {                          // include/bbai.h bbai_demo_chunk: the outputs of one bbai_bot_rollout call
    const uint8_t* image; const uint8_t* dir; const uint8_t* action; const uint8_t* tokens;
};

// bytes [sh, sh + 16) of the 32 bytes {lo, hi}, sh = 0..15.  Scalars only: a select between two elements of a private array becomes a
// dynamically indexed load, and the array then lives in scratch or LDS instead of registers.
__device__ __forceinline__ u32x4 demo_shr(const u32x4 lo, const u32x4 hi, uint32_t sh) {
    const bool d2 = (sh & 8u) != 0, d1 = (sh & 4u) != 0;
    const uint32_t b = sh & 3u;
    const uint32_t a0 = d2 ? lo.z : lo.x, a1 = d2 ? lo.w : lo.y, a2 = d2 ? hi.x : lo.z, a3 = d2 ? hi.y : lo.w, a4 = d2 ? hi.z : hi.x, a5 = d2 ? hi.w : hi.y;
    const uint32_t c0 = d1 ? a1 : a0, c1 = d1 ? a2 : a1, c2 = d1 ? a3 : a2, c3 = d1 ? a4 : a3, c4 = d1 ? a5 : a4;
    u32x4 w;
    w.x = __builtin_amdgcn_alignbyte(c1, c0, b);
    w.y = __builtin_amdgcn_alignbyte(c2, c1, b);
    w.z = __builtin_amdgcn_alignbyte(c3, c2, b);
    w.w = __builtin_amdgcn_alignbyte(c4, c3, b);
    return w;
}

// the 16 bytes at p (any byte phase): the two aligned 16-byte words around them.  All 16 bytes must be readable.
struct DemoWindow {
    u32x4 lo, hi; uint32_t phase;
    __device__ __forceinline__ void load(const uint8_t* p) {
        phase = (uint32_t)((uintptr_t)p & 15u);
        const u32x4* q = (const u32x4*)(p - phase);
        lo = q[0];
        hi = lo;
        if (phase) hi = q[1];                   // (phase 0: the second word may lie behind the allocation)
    }
    __device__ __forceinline__ u32x4 get() const {
        return demo_shr(lo, hi, phase);
    }
};

// One destination chunk: `a` alone (shift 0), or the last `16 - shift` bytes of the window `a` followed by the first
// `shift` bytes of the window `b` (a = the 16 bytes that END run A, b = the 16 bytes that BEGIN run B).
struct DemoPiece {
    DemoWindow a, b; uint32_t shift; bool two;
    __device__ __forceinline__ void load(const uint8_t* pa, const uint8_t* pb, uint32_t sh) {
        shift = sh; two = pb != nullptr;
        a.load(pa);
        if (two) b.load(pb);
    }
    __device__ __forceinline__ u32x4 get() const {
        const u32x4 wa = a.get();
        if (!two) return wa;
        const u32x4 wb = b.get();
        return demo_shr(wa, wb, shift);
    }
};

// aligned 16-byte store of chunk `q` of `dst`; the destination's last chunk may be short
__device__ __forceinline__ void demo_store(uint8_t* dst, int64_t q, const u32x4 v, int64_t total_bytes) {
    const int64_t left = total_bytes - q * 16;
    if (left >= 16) { ((u32x4*)dst)[q] = v; return; }
    for (int i = 0; i < (int)left; ++i) {
        const uint32_t w = i < 4 ? v.x : i < 8 ? v.y : i < 12 ? v.z : v.w;
        dst[q * 16 + i] = (uint8_t)(w >> (8 * (i & 3)));
    }
}

// index of the run that holds frame f: the largest k in [0, count) with start[k] <= f (start ascending, start[0] <= f)
__device__ __forceinline__ int64_t demo_find(const int64_t* __restrict__ start, int64_t count, int64_t f) {
    int64_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (start[mid] <= f) lo = mid; else hi = mid;
    }
    return lo;
}

// the same in the block's slice (frames relative to the block's first): the largest j with s_rel[j] <= x
__device__ __forceinline__ int demo_find_lds(const int32_t* s_rel, int x) {
    int j = 0;
#pragma unroll
    for (int step = DEMO_SLICE / 2; step > 0; step >>= 1)
        if (s_rel[j + step] <= x) j += step;
    return j;
}

// ------------------------------------------------------------------------------------------
// k_demo_spans : lane = stream (babyai_amd/demos.py scan_chunk, which stays this kernel's oracle).  done / gave_up / reward
// are [chunk][n]: at every t a wave reads 64 consecutive streams.  Carry per stream: last_done (global index of the latest
// episode end), open (still looking), span (first and last global step of the first solved episode).  open_count receives
// the number of streams still open after this chunk: one add per wave that has any (nobody waits for the sum).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_demo_spans(int64_t n, int chunk, const uint8_t* __restrict__ done, const uint8_t* __restrict__ gave_up,
                                                   const float* __restrict__ reward, int g0, int filter_steps, int32_t* __restrict__ last_done,
                                                   uint8_t* __restrict__ open, int32_t* __restrict__ span, unsigned long long* __restrict__ open_count) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    bool still = false;
    if (i < n) {
        int32_t last = last_done[i];
        const bool was_open = open[i] != 0;
        bool found = false;
        int32_t first = 0, at = 0;
        for (int t = 0; t < chunk; ++t) {
            const int64_t k = (int64_t)t * n + i;
            if (!done[k]) continue;
            const int32_t g = g0 + t;
            bool ok = gave_up[k] == 0 && reward[k] > 0.0f;
            if (filter_steps) ok = ok && (g - last) <= filter_steps;       // episode length = g - (last + 1) + 1
            if (ok && !found) { found = true; first = last + 1; at = g; }
            last = g;
        }
        last_done[i] = last;
        if (was_open && found) { span[2 * i] = first; span[2 * i + 1] = at; open[i] = 0; }
        still = was_open && !found;
    }
    const unsigned long long bal = __ballot(still);
    if (bal != 0ull && threadIdx.x == 0) atomicAdd(open_count, (unsigned long long)__popcll(bal));
}

// ------------------------------------------------------------------------------------------
// k_demo_jobs : lane = env of a POOL that plays a list of seeds, one episode per seed (DemoStore.collect_seeds: the listed-seed contract of
// scripts/train_intelligent_expert.py:106-147 generate_demos -- env.seed(s); env.reset(), the expert plays THAT episode, kept iff it ends with
// reward > 0 and without a bot exception).  job[i] = the position in the seed list env i is playing (-1: idle), start[i] = the global step its
// episode began at; episodes begin on a chunk's first row only (reseeds happen between chunks).  done / gave_up / reward are this chunk's
// [chunk][n], read as k_demo_spans reads them.  An env whose episode ends in this chunk -- the FIRST done row -- appends the record
// (env, first step, length, job) if the episode is kept, and claims the next unplayed job: ids_out[i] = i, seeds_out[i] = its seed for
// bbai_reseed, start[i] = the next chunk's first row; with the list exhausted it goes idle.  Every other env gets ids_out[i] = -1 (bbai_reseed
// skips it).  counters: [0] job cursor (in / out; may pass n_jobs by the claims that found nothing), [1] episodes finished (running total),
// [2] records and [3] frames of this call (zeroed by the entry).  Per wave: one ballot and one returning add for the claims, one for the
// records, one add each for the two totals -- none per lane, none in the row loop.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_demo_jobs(int64_t n, int chunk, const uint8_t* __restrict__ done, const uint8_t* __restrict__ gave_up,
                                                  const float* __restrict__ reward, int g0, int32_t* __restrict__ job, int32_t* __restrict__ start,
                                                  const uint64_t* __restrict__ job_seeds, int64_t n_jobs, int64_t* __restrict__ ids_out,
                                                  uint64_t* __restrict__ seeds_out, int32_t* __restrict__ rec, unsigned long long* __restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int lane = (int)threadIdx.x;
    bool fin = false, keep = false;
    int32_t mine = -1, first = 0, len = 0;
    if (i < n) {
        mine = job[i];
        if (mine >= 0) {
            for (int t = 0; t < chunk; ++t) {
                const int64_t k = (int64_t)t * n + i;
                if (!done[k]) continue;
                fin = true;
                keep = gave_up[k] == 0 && reward[k] > 0.0f;
                first = start[i];
                len = g0 + t - first + 1;
                break;
            }
        }
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long fin_bal = __ballot(fin), keep_bal = __ballot(keep);
    int sum = keep ? len : 0;                   // frames of the wave's kept episodes
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    unsigned long long job_base = 0, rec_base = 0;
    if (lane == 0) {
        if (fin_bal) {
            const unsigned long long c = (unsigned long long)__popcll(fin_bal);
            job_base = atomicAdd(counters, c);
            atomicAdd(counters + 1, c);
        }
        if (keep_bal) {
            rec_base = atomicAdd(counters + 2, (unsigned long long)__popcll(keep_bal));
            atomicAdd(counters + 3, (unsigned long long)sum);
        }
    }
    job_base = __shfl(job_base, 0);
    rec_base = __shfl(rec_base, 0);
    if (i >= n) return;
    if (keep) {
        int32_t* r = rec + 4 * (int64_t)(rec_base + (unsigned long long)__popcll(keep_bal & below));
        r[0] = (int32_t)i; r[1] = first; r[2] = len; r[3] = mine;
    }
    int64_t id = -1;
    if (fin) {
        const unsigned long long next = job_base + (unsigned long long)__popcll(fin_bal & below);
        if (next < (unsigned long long)n_jobs) {
            id = i;
            seeds_out[i] = job_seeds[next];
            job[i] = (int32_t)next;
            start[i] = g0 + chunk;
        } else {
            job[i] = -1;
        }
    }
    ids_out[i] = id;
}

// ------------------------------------------------------------------------------------------
// k_demo_replay_feed : a GROUP of 16 lanes = one env of a POOL that plays a store's demonstrations back (DemoStore.replay: DemoAgent of
// babyai/utils/agent.py:101-137, which asserts at every frame that the env shows the recorded observation).  Env i plays demo job[i] (< 0:
// nobody's) and stands at its frame pos[i]; it is FED iff 0 <= job < n_demos and 0 <= pos < the demo's length and the frame
// f = offset[job] + pos lies in [0, frames) -- anything else never becomes an address, and the env gets BBAI_ACTION_HOLD and fed = 0 with
// the results untouched.  A fed env's current observation (row i of `image` [n][147] and of `dir`) is compared with frame f of the store:
// lanes 0..9 of the group take the ten 16-byte windows [0,16) .. [128,144), [131,147) of the two 147-byte rows -- every window lies INSIDE
// its row, so the aligned 16-byte words around it (DemoWindow) stay inside an allocation that starts 16-byte aligned and is a multiple of 16
// bytes long, at any of the 16 byte phases of 147 i and 147 f; consecutive groups read consecutive env rows -- lane 10 the direction bytes,
// and at pos == 0 lanes 0..8 the nine 8-byte pieces of the two 72-byte token rows (both 8-byte aligned).  "Differs" is reduced by one ballot
// each; the group's lane 0 keeps the demo's books -- mismatches, first_mismatch (set while it is < 0), mission_ok at pos == 0 -- with plain
// loads and stores: one group owns one demo at a time.  It also writes actions_out[i] = the recorded action and fed[i] = 1.
// ------------------------------------------------------------------------------------------
constexpr int REPLAY_GROUP = 16;                // lanes per env
constexpr int REPLAY_ENVS = DEMO_BLOCK / REPLAY_GROUP;      // envs per block
constexpr uint8_t REPLAY_HOLD = 8;              // include/bbai.h BBAI_ACTION_HOLD

struct DemoReplayFeedArgs {
    int64_t n, n_demos, frames;
    const uint8_t* __restrict__ image; const uint8_t* __restrict__ dir; const uint8_t* __restrict__ tokens;       // the pool's current rows
    const int32_t* __restrict__ job; const int32_t* __restrict__ pos;
    const int64_t* __restrict__ offset;
    const uint8_t* __restrict__ s_image; const uint8_t* __restrict__ s_dir; const uint8_t* __restrict__ s_action; const uint8_t* __restrict__ s_tokens;
    int32_t* mismatches; int32_t* first_mismatch; uint8_t* mission_ok;
    uint8_t* actions_out; uint8_t* fed;
};

__device__ __forceinline__ bool demo_differs(const u32x4 a, const u32x4 b) {
    return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) != 0u;
}

__global__ __launch_bounds__(DEMO_BLOCK) void k_demo_replay_feed(DemoReplayFeedArgs a) {
    const int tid = threadIdx.x;
    const int sub = tid & (REPLAY_GROUP - 1);
    const int64_t i = (int64_t)blockIdx.x * REPLAY_ENVS + (tid >> 4);
    int64_t d = -1, f = 0;
    int32_t p = 0;
    if (i < a.n) {                              // (the group's 16 lanes read the same words: one broadcast load each)
        const int32_t j = a.job[i];
        p = a.pos[i];
        if (j >= 0 && (int64_t)j < a.n_demos && p >= 0) {
            const int64_t lo = a.offset[j], hi = a.offset[j + 1];
            f = lo + p;
            if (f < hi && f >= 0 && f < a.frames) d = j;
        }
    }
    const bool play = d >= 0;
    bool diff = false, tdiff = false;
    if (play) {
        if (sub < 10) {
            const uint32_t at = sub < 9 ? (uint32_t)sub * 16u : DEMO_ROW - 16u;
            DemoWindow we, ws;
            we.load(a.image + i * (int64_t)DEMO_ROW + at);
            ws.load(a.s_image + f * (int64_t)DEMO_ROW + at);
            diff = demo_differs(we.get(), ws.get());
        } else if (sub == 10) {
            diff = a.dir[i] != a.s_dir[f];
        }
        if (p == 0 && sub < 9) {
            const uint2 te = ((const uint2*)(a.tokens + i * 72))[sub], ts = ((const uint2*)(a.s_tokens + d * 72))[sub];
            tdiff = ((te.x ^ ts.x) | (te.y ^ ts.y)) != 0u;
        }
    }
    const int shift = (tid & 63) & ~(REPLAY_GROUP - 1);        // the group's first lane in its wave
    const bool any = ((__ballot(diff) >> shift) & 0xffffull) != 0ull;
    const bool tany = ((__ballot(tdiff) >> shift) & 0xffffull) != 0ull;
    if (sub != 0 || i >= a.n) return;
    if (play) {
        if (any) {
            a.mismatches[d] += 1;
            if (a.first_mismatch[d] < 0) a.first_mismatch[d] = p;
        }
        if (p == 0) a.mission_ok[d] = tany ? 0 : 1;
    }
    a.actions_out[i] = play ? a.s_action[f] : REPLAY_HOLD;
    a.fed[i] = play ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// k_demo_replay_judge : lane = env, behind the step that took k_demo_replay_feed's actions; modelled on k_demo_jobs.  It acts on FED envs
// only: a held env's done / reward64 entries are stale by the HOLD contract, and a reseeded env's done reads 1 until its first real step.  A
// fed env advances pos; with done set its demo's done_at = played = pos and return64 = the env's reward64, bit for bit; with the demo used up
// and no done, played = pos, done_at = 0, return64 = 0.0; either way the env gives its demo up (job = -1: WAITING, which is what idle is).
// With claim != 0 every env with job < 0 -- those that finished just now included -- claims the next position of the job list: one ballot
// and one returning add per wave, none per lane; position k < n_jobs gives job = job_demo[k] (k itself where job_demo is null), pos = 0,
// ids_out[i] = i and seeds_out[i] = job_seeds[k] for bbai_reseed; every other env gets ids_out[i] = -1.  With claim == 0 nothing is
// claimed and ids_out / seeds_out are not touched.  counters: [0] job cursor (in / out; may pass n_jobs by the claims that found nothing),
// [1] demos finished (running total; one add per wave that has any).
// ------------------------------------------------------------------------------------------
struct DemoReplayJudgeArgs {
    int64_t n, n_demos, n_jobs; int claim;
    const uint8_t* __restrict__ fed; const uint8_t* __restrict__ done; const double* __restrict__ reward64;
    int32_t* job; int32_t* pos;
    const int64_t* __restrict__ offset;
    int32_t* played; int32_t* done_at; double* return64;
    const int32_t* __restrict__ job_demo; const uint64_t* __restrict__ job_seeds;
    int64_t* ids_out; uint64_t* seeds_out; unsigned long long* counters;
};

__global__ __launch_bounds__(64) void k_demo_replay_judge(DemoReplayJudgeArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int lane = (int)threadIdx.x;
    bool fin = false, want = false;
    if (i < a.n) {
        int32_t j = a.job[i];
        if (a.fed[i] != 0 && j >= 0 && (int64_t)j < a.n_demos) {
            const int32_t p = a.pos[i] + 1;
            a.pos[i] = p;
            const bool dn = a.done[i] != 0;
            if (dn || (int64_t)p >= a.offset[j + 1] - a.offset[j]) {
                a.played[j] = p;
                a.done_at[j] = dn ? p : 0;
                a.return64[j] = dn ? a.reward64[i] : 0.0;
                a.job[i] = j = -1;
                fin = true;
            }
        }
        want = a.claim != 0 && j < 0;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long fin_bal = __ballot(fin), want_bal = __ballot(want);
    unsigned long long base = 0;
    if (lane == 0) {
        if (fin_bal) atomicAdd(a.counters + 1, (unsigned long long)__popcll(fin_bal));
        if (want_bal) base = atomicAdd(a.counters, (unsigned long long)__popcll(want_bal));
    }
    base = __shfl(base, 0);
    if (i >= a.n || a.claim == 0) return;
    int64_t id = -1;
    if (want) {
        const unsigned long long next = base + (unsigned long long)__popcll(want_bal & below);
        if (next < (unsigned long long)a.n_jobs) {
            id = i;
            a.seeds_out[i] = a.job_seeds[next];
            a.job[i] = a.job_demo ? a.job_demo[next] : (int32_t)next;
            a.pos[i] = 0;
        }
    }
    a.ids_out[i] = id;
}

// ------------------------------------------------------------------------------------------
// k_demo_pack : blocks [0, img_blocks) copy the frames (8 KiB of the store's image array each), the blocks behind them
// write direction / action (lane = 4 frames, one aligned dword of each) and the token rows (lane = 8 of a row's 72 bytes).
// Frame f of the store = history row g = span[k][0] + (f - offset[k]) of stream k, i.e. row g % T of chunk g / T.
// ------------------------------------------------------------------------------------------
struct DemoPackArgs {
    int64_t n, frames; int T; int64_t img_blocks, meta_blocks;
    const DemoChunkPtrs* __restrict__ chunks; const int32_t* __restrict__ span; const int64_t* __restrict__ offset;
    uint8_t* image; uint8_t* dir; uint8_t* action; uint8_t* tokens;
    // demo k lies in stream k, its first history row is span[k][0], chunk q of the history is entry q of the table
    __device__ __forceinline__ int64_t streams() const { return n; }
    __device__ __forceinline__ int64_t stream(int64_t k) const { return k; }
    __device__ __forceinline__ int32_t first(int64_t k) const { return span[2 * k]; }
    __device__ __forceinline__ int slot(int q) const { return q; }
};

// The list form (bbai_demo_pack_list): demo k is the record rec[k] = (stream, first step, length, job) that k_demo_jobs appended, and
// the history is a RING of R chunks: global row g is row g % T of entry (g / T) % R of the table.
struct DemoPackListArgs {
    int64_t n, frames; int T; int64_t img_blocks, meta_blocks;
    const DemoChunkPtrs* __restrict__ chunks; const int32_t* __restrict__ rec; const int64_t* __restrict__ offset;
    uint8_t* image; uint8_t* dir; uint8_t* action; uint8_t* tokens;
    int64_t n_streams; int R;
    __device__ __forceinline__ int64_t streams() const { return n_streams; }
    __device__ __forceinline__ int64_t stream(int64_t k) const { return rec[4 * k]; }
    __device__ __forceinline__ int32_t first(int64_t k) const { return rec[4 * k + 1]; }
    __device__ __forceinline__ int slot(int q) const { return q % R; }
};

template <class Args>
__device__ __forceinline__ int64_t demo_pack_row(const Args& a, int64_t k, int64_t g, int& c) {
    const int q = (int)(g / a.T);
    c = a.slot(q);
    return (g - (int64_t)q * a.T) * a.streams() + a.stream(k);
}

// source address of frame `rel` (relative to the block's first frame) in the history
template <class Args>
__device__ __forceinline__ const uint8_t* demo_pack_src(const Args& a, const int32_t* s_rel, const int32_t* s_g0, int64_t k_lo, int rel) {
    const int j = demo_find_lds(s_rel, rel);
    int c;
    const int64_t row = demo_pack_row(a, k_lo + j, (int64_t)s_g0[j] + (rel - s_rel[j]), c);
    return a.chunks[c].image + row * DEMO_ROW;
}

// the piece of the chunk at byte x relative to the block's first frame f_lo
template <class Args>
__device__ __forceinline__ void demo_pack_piece(const Args& a, DemoPiece& p, const int32_t* s_rel, const int32_t* s_g0, int64_t k_lo,
                                                int64_t f_lo, uint32_t x) {
    const uint32_t fr = __umulhi(x, DEMO_DIV147), r = x - fr * DEMO_ROW;
    const uint8_t* s0 = demo_pack_src(a, s_rel, s_g0, k_lo, (int)fr);
    if (r + 16 <= DEMO_ROW) { p.load(s0 + r, nullptr, 0); return; }
    const uint8_t* tail = s0 + DEMO_ROW - 16;
    const uint8_t* s1 = f_lo + fr + 1 < a.frames ? demo_pack_src(a, s_rel, s_g0, k_lo, (int)fr + 1) : tail;      // (behind the store's last frame: filler, never stored)
    p.load(tail, s1, 16 - (DEMO_ROW - r));
}

template <class Args>
__device__ __forceinline__ void demo_pack_body(const Args& a) {
    __shared__ int32_t s_rel[DEMO_SLICE + 1];   // first frame of the block's demos, relative to the block's first frame
    __shared__ int32_t s_g0[DEMO_SLICE];        // span[k][0] of those demos
    __shared__ int64_t s_klo;                   // the first of them
    const int tid = threadIdx.x;
    const int64_t blk = blockIdx.x;
    if (blk >= a.img_blocks + a.meta_blocks) {  // token rows: 9 pieces of 8 bytes per demo (both sides are 8-byte aligned)
        const int64_t p = (blk - a.img_blocks - a.meta_blocks) * DEMO_BLOCK + tid;
        const int64_t k = p / 9;
        if (k >= a.n) return;
        int c;
        const int64_t row = demo_pack_row(a, k, a.first(k), c);
        const int piece = (int)(p - k * 9);
        ((uint2*)a.tokens)[p] = ((const uint2*)(a.chunks[c].tokens + row * 72))[piece];
        return;
    }
    if (blk >= a.img_blocks) {                  // direction / action: 4 frames per lane
        const int64_t f0 = ((blk - a.img_blocks) * DEMO_BLOCK + tid) * 4;
        if (f0 >= a.frames) return;
        int64_t k = demo_find(a.offset, a.n, f0);
        uint32_t d = 0, act = 0;
        const int cnt = (int)(a.frames - f0 < 4 ? a.frames - f0 : 4);
        for (int i = 0; i < cnt; ++i) {
            const int64_t f = f0 + i;
            while (a.offset[k + 1] <= f) ++k;
            int c;
            const int64_t row = demo_pack_row(a, k, a.first(k) + (f - a.offset[k]), c);
            d |= (uint32_t)a.chunks[c].dir[row] << (8 * i);
            act |= (uint32_t)a.chunks[c].action[row] << (8 * i);
        }
        if (cnt == 4) { ((uint32_t*)a.dir)[f0 >> 2] = d; ((uint32_t*)a.action)[f0 >> 2] = act; }
        else for (int i = 0; i < cnt; ++i) { a.dir[f0 + i] = (uint8_t)(d >> (8 * i)); a.action[f0 + i] = (uint8_t)(act >> (8 * i)); }
        return;
    }
    const int64_t total = a.frames * (int64_t)DEMO_ROW;
    const int64_t byte0 = blk * DEMO_BLOCK_BYTES;
    const int64_t f_lo = byte0 / DEMO_ROW;
    const uint32_t r_lo = (uint32_t)(byte0 - f_lo * DEMO_ROW);
    if (tid < 64) {                             // the block's slice of `offset` (wave 0; the search is wave-uniform)
        const int64_t k0 = demo_find(a.offset, a.n, f_lo);
        const int64_t k = k0 + tid;
        const int64_t rel = k <= a.n ? a.offset[k] - f_lo : (int64_t)0x7fffffff;
        s_rel[tid] = (int32_t)(rel < 0x7fffffff ? rel : 0x7fffffff);
        s_g0[tid] = k < a.n ? a.first(k) : 0;
        if (tid == 0) { s_rel[DEMO_SLICE] = 0x7fffffff; s_klo = k0; }
    }
    __syncthreads();
    const int64_t k_lo = s_klo;
    // the two chunks of a lane as two named pieces (no arrays: everything stays in registers); both pieces' loads are issued
    // before the first store
    const int64_t q0 = blk * (DEMO_BLOCK * DEMO_UNROLL) + tid, q1 = q0 + DEMO_BLOCK;
    const bool v0 = q0 * 16 < total, v1 = q1 * 16 < total;
    DemoPiece p0, p1;
    if (v0) demo_pack_piece(a, p0, s_rel, s_g0, k_lo, f_lo, r_lo + (uint32_t)tid * 16u);
    if (v1) demo_pack_piece(a, p1, s_rel, s_g0, k_lo, f_lo, r_lo + (uint32_t)(DEMO_BLOCK + tid) * 16u);
    if (v0) demo_store(a.image, q0, p0.get(), total);
    if (v1) demo_store(a.image, q1, p1.get(), total);
}

__global__ __launch_bounds__(DEMO_BLOCK) void k_demo_pack(DemoPackArgs a) { demo_pack_body(a); }
__global__ __launch_bounds__(DEMO_BLOCK) void k_demo_pack_list(DemoPackListArgs a) { demo_pack_body(a); }

// ------------------------------------------------------------------------------------------
// k_demo_batch : the batch gather.  order[b] = the store's demo that comes b-th, dst_start[b] its first frame in the result
// (int64[B + 1], the last entry = the result's frame count), offset = the store's.  Blocks [0, img_blocks) copy the images
// (the bytes of demo order[b] are one contiguous run on both sides, at any byte phase on both sides); the blocks behind them
// write the per-frame fields, 4 frames per lane: batch form (action int64, done, mask float32, episode_ids int64 non-null:
// imitation.py:240-250) or store form (dir / action uint8: DemoStore.select).
// ------------------------------------------------------------------------------------------
struct DemoBatchArgs {
    int64_t B, frames, img_blocks;
    const int64_t* __restrict__ order; const int64_t* __restrict__ dst_start; const int64_t* __restrict__ offset;
    const uint8_t* __restrict__ src_image; const uint8_t* __restrict__ src_dir; const uint8_t* __restrict__ src_action;
    uint8_t* image; int64_t* action64; uint8_t* done; float* mask; int64_t* episode; uint8_t* dir8; uint8_t* action8;
};

// the piece of the chunk at byte x relative to the block's first frame f_lo (destination byte `base`)
__device__ __forceinline__ void demo_batch_piece(const DemoBatchArgs& a, DemoPiece& p, const int32_t* s_rel, const int64_t* s_delta, int64_t f_lo,
                                                 int64_t base, uint32_t x) {
    const int fr = (int)__umulhi(x, DEMO_DIV147);
    const int j = demo_find_lds(s_rel, fr);
    const int64_t end_rel = (int64_t)s_rel[j + 1] * DEMO_ROW;              // where demo j ends, relative to frame f_lo (int64: the sentinel is large)
    const uint8_t* sa = a.src_image + base + s_delta[j] * (int64_t)DEMO_ROW;      // source byte of "relative byte 0" for demo j
    if ((int64_t)x + 16 <= end_rel) { p.load(sa + x, nullptr, 0); return; }
    const uint8_t* tail = sa + end_rel - 16;
    const bool next = s_rel[j + 1] + f_lo < a.frames;                      // (behind the result's last demo: filler, never stored)
    p.load(tail, next ? a.src_image + base + s_delta[j + 1] * (int64_t)DEMO_ROW + end_rel : tail, (uint32_t)(16 - (end_rel - x)));
}

__global__ __launch_bounds__(DEMO_BLOCK) void k_demo_batch(DemoBatchArgs a) {
    __shared__ int32_t s_rel[DEMO_SLICE + 1];   // first frame of the block's demos in the result, relative to the block's first frame
    __shared__ int64_t s_delta[DEMO_SLICE];     // source frame - destination frame of those demos
    const int tid = threadIdx.x;
    const int64_t blk = blockIdx.x;
    if (blk >= a.img_blocks) {
        const int64_t f0 = ((blk - a.img_blocks) * DEMO_BLOCK + tid) * 4;
        if (f0 >= a.frames) return;
        int64_t b = demo_find(a.dst_start, a.B, f0);
        const int cnt = (int)(a.frames - f0 < 4 ? a.frames - f0 : 4);
        int64_t act[4], ep[4]; float m[4]; uint32_t dn = 0, d8 = 0, a8 = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            act[i] = 0; ep[i] = 0; m[i] = 0.0f;
            if (i >= cnt) continue;
            const int64_t f = f0 + i;
            while (a.dst_start[b + 1] <= f) ++b;
            const int64_t s = a.offset[a.order[b]] + (f - a.dst_start[b]);
            const uint32_t av = a.src_action[s];
            act[i] = (int64_t)av; ep[i] = b; m[i] = f == a.dst_start[b] ? 0.0f : 1.0f;
            dn |= (uint32_t)(f + 1 == a.dst_start[b + 1]) << (8 * i);
            a8 |= av << (8 * i);
            if (a.dir8) d8 |= (uint32_t)a.src_dir[s] << (8 * i);
        }
        if (cnt == 4) {
            if (a.action64) {
                typedef int64_t i64x2 __attribute__((ext_vector_type(2)));
                typedef float f32x4 __attribute__((ext_vector_type(4)));
                i64x2* ao = (i64x2*)(a.action64 + f0); i64x2* eo = (i64x2*)(a.episode + f0);
                ao[0] = i64x2{act[0], act[1]}; ao[1] = i64x2{act[2], act[3]};
                eo[0] = i64x2{ep[0], ep[1]}; eo[1] = i64x2{ep[2], ep[3]};
                *(f32x4*)(a.mask + f0) = f32x4{m[0], m[1], m[2], m[3]};
                ((uint32_t*)a.done)[f0 >> 2] = dn;
            } else {
                ((uint32_t*)a.dir8)[f0 >> 2] = d8; ((uint32_t*)a.action8)[f0 >> 2] = a8;
            }
        } else
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i >= cnt) break;
            if (a.action64) { a.action64[f0 + i] = act[i]; a.episode[f0 + i] = ep[i]; a.mask[f0 + i] = m[i]; a.done[f0 + i] = (uint8_t)(dn >> (8 * i)); }
            else { a.dir8[f0 + i] = (uint8_t)(d8 >> (8 * i)); a.action8[f0 + i] = (uint8_t)(a8 >> (8 * i)); }
        }
        return;
    }
    const int64_t total = a.frames * (int64_t)DEMO_ROW;
    const int64_t byte0 = blk * DEMO_BLOCK_BYTES;
    const int64_t f_lo = byte0 / DEMO_ROW;
    const int64_t base = f_lo * DEMO_ROW;       // destination byte of the block's first frame
    const uint32_t r_lo = (uint32_t)(byte0 - base);
    if (tid < 64) {
        const int64_t b_lo = demo_find(a.dst_start, a.B, f_lo);
        const int64_t b = b_lo + tid;
        const int64_t rel = b <= a.B ? a.dst_start[b] - f_lo : (int64_t)0x7fffffff;
        s_rel[tid] = (int32_t)(rel < 0x7fffffff ? rel : 0x7fffffff);
        s_delta[tid] = b < a.B ? a.offset[a.order[b]] - a.dst_start[b] : 0;
        if (tid == 0) s_rel[DEMO_SLICE] = 0x7fffffff;
    }
    __syncthreads();
    const int64_t q0 = blk * (DEMO_BLOCK * DEMO_UNROLL) + tid, q1 = q0 + DEMO_BLOCK;
    const bool v0 = q0 * 16 < total, v1 = q1 * 16 < total;
    DemoPiece p0, p1;
    if (v0) demo_batch_piece(a, p0, s_rel, s_delta, f_lo, base, r_lo + (uint32_t)tid * 16u);
    if (v1) demo_batch_piece(a, p1, s_rel, s_delta, f_lo, base, r_lo + (uint32_t)(DEMO_BLOCK + tid) * 16u);
    if (v0) demo_store(a.image, q0, p0.get(), total);
    if (v1) demo_store(a.image, q1, p1.get(), total);
}

}  // namespace bbai
