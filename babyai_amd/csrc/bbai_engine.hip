// bbai_engine.hip -- the host side and the C ABI of the batched BabyAI engine (gfx950 / MI355X): the handle (bbai_env), its options, the
// launches of every kernel and the streams, windows and events around them.  This file holds no kernel; its translation unit is made of
// the kernel headers it includes, one per family, each at the spot where its code stood (the order is the kernels' order in the library,
// nothing else: every header includes what it uses; what several families or this file share is in bbai_kernels.hpp).
//
// Kernels (all integer / byte work, HBM- and latency-bound; no MFMA by design) -- where each one lives:
//   bbai_stepk.hpp    k_step<VP, FUSE, CP>, k_step_ticks: lane = env, one wave per block; the finished envs' consume (consume_env,
//                     advance_load / advance_finish) and the step's dirty cells for its delta render (step_dirty).  Launched by step_kernel.
//   bbai_pregen.hpp   k_pregen<F, G, OBS>: the lane-group level generator, one env per group of G lanes, into the env's look-ahead ring;
//                     k_mt_sync / k_mt_canon: the two forms of the generators' RNG state.  (launch_pregen_g, mt_sync, mt_canon.  The lane =
//                     level generator k_pregen_lane is bbai_genlane.hip, a translation unit of its own: launch_pregen_lane -> bbai_lane_launch.)
//   bbai_ring.hpp     k_consume (look-ahead slot -> live state over the reset list: unfused steps, reset()); k_compact / k_mark / k_gate (the
//                     windows' turnover: window_begin, window_end); k_probe_wait / k_probe_set (probe_stream); k_live_copy, k_import_hot,
//                     k_sync_prog / k_sync_view / k_sync_cpl (export, import, checkpoints); k_seed, k_init_hot.
//   bbai_botk.hpp     k_bot<W>: one decision of the reference's expert per env (bbai_bot.hpp); k_botg in experiment builds.  (bot_launch)
//   bbai_render.hpp   k_render_q / k_render: RGBImgPartialObsWrapper as a pure tile-atlas gather: atlas + per-cell tile ids in LDS, 16 bytes per
//                     lane per store, a wave writes 1 KiB of contiguous pixels; persistent blocks fed by ONE ticket counter from 262 144 envs
//                     (k_render_q), one-shot (512, 2) blocks below.  Into the registered target (bbai_set_render_target): k_render_delta /
//                     k_render_dstore, the delta render -- only the 64-byte pieces (or 128-byte lines) whose cells changed since the frame
//                     the buffer holds are stored.  (render_launch)
//   bbai_gridk.hpp    k_render_grid<TS>: the full-grid picture; k_full_obs: the fully observable encoding.  (render_grid_launch, full_launch)
//   bbai_griddelta.hpp k_grid_delta<TS>: the full-grid picture of the whole batch into the registered grid target (include/bbai_grid_target.h), only the
//                     64-byte pieces that hold a changed cell; k_grid_ids: every tile id behind a whole-frame render into it.  (grid_target_launch)
//   bbai_viewn.hpp    k_view_obs<V>: the egocentric observation at view sizes 3 .. 11 (ViewSizeWrapper).  (viewn_launch)
//   bbai_viewpx.hpp   k_view_pixels<TS>: the 7x7 view as pixels at tile sizes 16 / 32 (render_view_launch); k_view_delta<TS> / k_view_ids: a whole
//                     batch into the target registered at that size, only the 64-byte pieces whose cells changed.  (view_delta_launch)
//   bbai_viewpxn.hpp  k_view_pixels_n<V, TS>: the V x V view as pixels, view sizes 3 .. 11 at tile sizes 8 / 16 / 32, of rows of an encoded
//                     buffer (include/bbai_view_pixels.h).  (view_pixels_launch)
//   bbai_tokens.hpp   k_tokens: mission text as fixed-vocabulary token ids of the envs that started a new episode (window_end); k_tap (tap_launch);
//                     k_gae (bbai_gae).
//   bbai_demo.hpp     k_demo_spans / k_demo_pack / k_demo_batch / k_demo_jobs / k_demo_pack_list: demonstrations that stay on the device;
//                     k_demo_replay_feed / k_demo_replay_judge: a pool of envs plays them back (include/bbai_demo_replay.h).
//   bbai_statek.hpp   k_state_save / k_state_load / k_state_tokens: device snapshots of listed envs (bbai_save_state, bbai_load_state).
//   bbai_reseedk.hpp  k_reseed_seed / k_reseed_consume: env.seed(s); env.reset() for listed envs of a live batch (bbai_reseed).
//
// Reference semantics: see bbai_step.hpp / bbai_gen.hpp / bbai_bot.hpp headers for file:line citations.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include <type_traits>
#include <vector>

#if defined(BBAI_BOT_PROF)
__device__ unsigned long long g_bot_prof[32];        // experiment builds: phase timers of the expert (bbai_bot.hpp)
#endif
#include "../../include/bbai.h"
#include "../../include/bbai_demo_replay.h"
#include "../../include/bbai_view_size.h"
#include "../../include/bbai_view_pixels.h"
#include "../../include/bbai_grid_target.h"
#include "bbai_types.hpp"
#include "bbai_target.hpp"
#include "bbai_gridtarget.hpp"
#include "bbai_kernels.hpp"
#include "bbai_gen.hpp"
#include "bbai_genl.hpp"
#include "bbai_step.hpp"
#include "bbai_view.hpp"
#include "bbai_grid.hpp"
#include "bbai_bot.hpp"
#include "bbai_seed.hpp"

using namespace bbai;

static_assert(sizeof(bbai_level_cfg) == sizeof(LevelCfg), "C ABI cfg mirrors bbai::LevelCfg");

static thread_local char g_err[512] = "";
static thread_local hipError_t g_hip = hipSuccess;      // the HIP error behind the latest BBAI_ERR_HIP (for callers that word the failure themselves)
#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            g_hip = e_;                                                                       \
            snprintf(g_err, sizeof(g_err), "%s:%d %s -> %s", __FILE__, __LINE__, #expr,       \
                     hipGetErrorString(e_));                                                  \
            return BBAI_ERR_HIP;                                                              \
        }                                                                                     \
    } while (0)
// ... and for the helpers below that return a BBAI_* code (g_err was written where it failed)
#define BBAI_TRY(expr)                                                                        \
    do {                                                                                      \
        int rc_ = (expr);                                                                     \
        if (rc_ != BBAI_OK) return rc_;                                                       \
    } while (0)

#define ARG_FAIL(msg)                                                                        \
    do {                                                                                      \
        snprintf(g_err, sizeof(g_err), "%s: %s", __func__, msg);                              \
        return BBAI_ERR_ARG;                                                                  \
    } while (0)

// Entry points run on the handle's device but must leave the caller's current device alone (torch tracks the
// HIP current device of the thread; a library that changes it redirects the caller's later allocations).
struct DeviceGuard {
    int prev = -1, err = hipSuccess;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev); else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define ON_DEVICE(dev)                                                                        \
    DeviceGuard guard_(dev);                                                                  \
    HIP_TRY((hipError_t)guard_.err)

// What a handle holds -- device memory, the pinned host words, streams, events -- is made and let go by the helpers between the two markers below, the
// only raw allocation / creation calls of this file (tests/test_handle_owner_source.py); none of them launches anything.
//   Scoped   one resource that dies with its scope unless a field of the handle adopts it: a call's temporaries, and the way a feature gets its
//            buffers all or none -- the whole group as Scoped, adopted once every piece exists;
//   Owner    the handle's record: the address of every field that holds a resource right now (the handle lives on the heap and never moves).
// ---- owner helpers: begin
enum ResKind : uint8_t { RES_MEM, RES_PINNED, RES_STREAM, RES_EVENT };
static int res_done(const char* call, hipError_t r) {             // BBAI_OK -- or g_err and g_hip written, BBAI_ERR_HIP
    if (r != hipSuccess) snprintf(g_err, sizeof(g_err), "%s: %s -> %s", __FILE__, call, hipGetErrorString(g_hip = r));
    return r == hipSuccess ? BBAI_OK : BBAI_ERR_HIP;
}
static hipError_t res_release(ResKind k, void* h) { return k == RES_MEM ? hipFree(h) : k == RES_PINNED ? hipHostFree(h) : k == RES_STREAM ? hipStreamDestroy((hipStream_t)h) : hipEventDestroy((hipEvent_t)h); }
struct Scoped {
    ResKind kind = RES_MEM; void* h = nullptr;
    Scoped() = default; Scoped(const Scoped&) = delete; Scoped& operator=(const Scoped&) = delete;
    ~Scoped() { reset(); }
    void reset() { if (h) (void)res_release(kind, h); h = nullptr; }
    int mem(size_t bytes, bool zero = false) {                   // device memory, zeroed where asked
        const hipError_t r = hipMalloc(&h, bytes);
        return r == hipSuccess && zero ? res_done("hipMemset", hipMemset(h, 0, bytes)) : res_done("hipMalloc", r);
    }
    int pinned(size_t bytes) { kind = RES_PINNED; return res_done("hipHostMalloc", hipHostMalloc(&h, bytes, hipHostMallocMapped)); }      // mapped pinned host memory
    int stream(unsigned flags, const int* prio = nullptr) {      // the flags form, or the priority form
        kind = RES_STREAM;
        return res_done("hipStreamCreate", prio ? hipStreamCreateWithPriority((hipStream_t*)&h, flags, *prio) : hipStreamCreateWithFlags((hipStream_t*)&h, flags));
    }
    int event(unsigned flags = hipEventDisableTiming) {          // (hipEventDefault: the timing pairs of bbai_profile)
        kind = RES_EVENT;
        return res_done("hipEventCreate", flags == hipEventDefault ? hipEventCreate((hipEvent_t*)&h) : hipEventCreateWithFlags((hipEvent_t*)&h, flags));
    }
};
struct Owner {
    struct Held { ResKind kind; void* field; }; struct Want { void* field; size_t bytes; bool zero; };
    std::vector<Held> held;            // every field of the handle that holds a resource right now, in the order they got it
    template <class T> void adopt(T* field, Scoped& t) { if (t.h) { *field = (T)t.h; held.push_back({t.kind, (void*)field}); t.h = nullptr; } }      // (into an empty field; an empty temporary is passed over)
    int alloc(std::initializer_list<Want> wants) {               // device memory into empty fields, in the order given: all of them or none
        std::vector<Scoped> t(wants.size());
        size_t i = 0, k = 0;
        for (const Want& w : wants) BBAI_TRY(t[i++].mem(w.bytes, w.zero));
        for (const Want& w : wants) adopt((void**)w.field, t[k++]);
        return BBAI_OK;
    }
    int stream(hipStream_t* field, unsigned flags, const int* prio = nullptr) { Scoped t; BBAI_TRY(t.stream(flags, prio)); adopt(field, t); return BBAI_OK; }
    int event(hipEvent_t* field, unsigned flags = hipEventDisableTiming) { Scoped t; BBAI_TRY(t.event(flags)); adopt(field, t); return BBAI_OK; }
    int drop(void* field) {                                      // release what the field holds (nothing: fine) and null it
        for (size_t i = held.size(); i-- > 0;) if (held[i].field == field) {
            const ResKind kind = held[i].kind;
            void* h = nullptr;
            memcpy(&h, field, sizeof(h)); memset(field, 0, sizeof(h));          // (fields are pointers of many types: read and nulled as bytes)
            held.erase(held.begin() + (long)i);
            return res_done("release", res_release(kind, h));
        }
        return BBAI_OK;
    }
    void drop_all() { while (!held.empty()) (void)drop(held.back().field); }       // bbai_destroy: the latest first
};
// ---- owner helpers: end

constexpr int PROF_RING = 256;          // event pairs per profiled kernel (bbai_profile)
constexpr int MAX_SIDES = 8;            // look-ahead streams a window's refill can be split over
#ifndef LOOKAHEAD_STREAMS_DEFAULT
#define LOOKAHEAD_STREAMS_DEFAULT 1
#endif
constexpr int MAX_PERIOD = 96;          // refill period B (ticks per look-ahead refill); ring depth D = 2B (+ 1 in place): slot numbers and per-window counts stay bytes

struct bbai_env {       // (the int knobs' option names, BBAI_* variables, defaults and clamps: KNOBS, below)
    LevelCfg cfg;
    int64_t n;
    int device;
    uint8_t* rec;         // [n][rec_bytes]
    Hot* hot;             // [n]
    uint64_t* stale;      // [n]
    uint32_t* mt;         // [n][624]
    int32_t* mti;         // [n]
    uint32_t* vhead;      // [n]     verifier program head (SoA, see VProg)
    uint64_t* vset;       // [8][n]  obj_set bitmasks, k = 2*leaf + slot
    // Look-ahead ring of depth D = 2B: every env owns D pre-generated levels; a finished env consumes slot hot.slot.
    // Consume-ticks are grouped into windows of B ticks; the slots consumed during window w are refilled by ONE
    // k_pregen launch at the end of the window (so the generator's slowest level is paid once per B ticks), and
    // that refill only has to land before window w+2 starts (worst case an env consumes one slot per tick).
    int depth, period;    // D, B
    uint8_t* next_rec;    // [D][n][rec_bytes]
    Hot* next_hot;        // [D][n]
    uint8_t* next_obs;    // [D][n][OBS_SLOT] in-place layout only: the first observation of every look-ahead level, written by the generator
    uint8_t* pending;     // [NWIN][n]  per window buffer: slots consumed by env in the window (0 = not in the window)
    uint8_t* first_slot;  // [NWIN][n]  first slot the env freed in the window
    uint32_t* win_meta;   // [NWIN][META_U32] one 128-byte line per window buffer (k_gate; the consume paths' atomicMax)
    unsigned long long* totals;   // [SHARDS][SHARD_U64] resets so far, sharded over cache lines (sum = bbai_reset_count)
    unsigned long long* flow;     // [FLOW_WORDS] refilled windows, gate time-outs, generator give-ups
    int32_t* gen_list;    // [SHARDS][gen_sublist_cap(n)] the refill's work list (look-ahead stream only): k_compact -> k_pregen
    uint32_t* gen_count;  // [SHARDS][GEN_COUNT_U32] its sub-list lengths
    int32_t* reset_list;  // [n]     unfused consume only: envs finished by the current step (k_step<.., 0> -> k_consume / k_tokens)
    uint8_t* reset_slot;  // [n]     ... and the look-ahead slot each of them consumes (spares k_consume one dependent round trip)
    uint32_t* counters;   // [2][16] [p][0] = reset list length; ping-pong by step parity so that k_consume can zero the
                          //         other one for the next step (no memset launch on the step path)
    int step_parity;
    bool next_counter_clean;
    uint8_t* tokens;      // optional caller-owned [n][72] mission token buffer kept current on resets
    hipStream_t side;     // look-ahead generation stream (= sides[0]: bbai_seed's first fill, the probe)
    // Round 6: a window's refill is split over n_sides look-ahead streams, each with a CONTIGUOUS range of 64-env blocks and a work list of its own.
    // An env's levels are generated in stream order on ITS stream (its MT19937 state never has two writers); the streams run side by side, so
    // refill w + 1 of one range starts while refill w of another is still at its slowest level.  k_mark runs on a stream of its own behind an
    // event of every part (`refilled` stays "every env of windows < r has its levels").
    hipStream_t sides[MAX_SIDES];
    hipStream_t mark_stream;
    hipEvent_t ev_part[MAX_SIDES];
    int side_prio;
    int n_sides;          // look-ahead streams in use (set_sides)
    int32_t* gen_lists[MAX_SIDES];      // sides >= 1 (side 0: gen_list / gen_count below)
    uint32_t* gen_counts[MAX_SIDES];
    hipStream_t split;    // bbai_step_render: the second half-batch's k_step runs here, under the first half's render
    hipEvent_t ev_split0, ev_splitB;
    int step_render_split;   // 1 = split (from STEP_RENDER_SPLIT_MIN envs), 0 = never, -1 = default
    hipEvent_t ev_consumed;
    hipEvent_t ev_refill[NWIN];     // recorded behind every window's refill; only waited for in strict mode (below) -- k_gate reads flow[FLOW_REFILLED]
    int gate_strict;      // 1 = rounds 1-4's rule as well: the stream waits (an event) for the refill of window
                          // x - 2 before window x starts, so k_gate never has to wait (A/B runs; a fallback should a profiler serialise the two streams)
    // The relaxed gate is a device-side spin on a value the look-ahead stream's k_mark stores: it relies on kernels of the two streams making
    // progress CONCURRENTLY, which HIP does not promise (streams can share a hardware queue; a profiler can serialise launches).  So:
    //   * the first window a caller's stream opens PROBES it (probe_stream: a waiting kernel on the caller's stream, the releasing one on the
    //     look-ahead stream behind it); a stream that fails runs under the strict rule (event waits, k_gate never has to wait) from then on;
    //   * a gate that gives up all the same sets a sticky word in pinned host memory, which every entry point reads before it enqueues anything:
    //     the handle refuses to step on (BBAI_ERR_STATE) instead of consuming slots that were never refilled.
    volatile uint32_t* host_flags;    // pinned, mapped: [0] a window gate timed out (sticky)  [1] the last probe's verdict (1 concurrent, 2 not)
    uint32_t* host_flags_dev;         // the device's address of the same words
    hipStream_t probed[8];            // caller streams already probed ...
    bool probed_ok[8];                // ... and what the probe said
    int n_probed;
    int gate_probe;                   // 1 (default) = probe, 0 = trust the streams (no probe), 2 = treat every probe as failed (tests)
    int gate_forced;                  // the current caller stream failed the probe: strict rule
    hipStream_t last_stream;   // the caller's stream of the previous call (compared, never used): a handle follows ONE stream
    bool have_stream;          // at a time; a call on another stream waits for ev_switch = end of the previous call
    hipEvent_t ev_switch;      // (enter_call / leave_call)
    bool call_events;
    int render_tpb;       // 256 / 512 / 1024 threads per render block; anything else = by batch size
    int render_group;     // 2, 4 or 8 envs per one-shot render block; anything else = by batch size (bbai_render)
    int pregen_cap;       // "pregen_blocks": upper bound on look-ahead lane groups per launch (experiments)
    int pregen_per_group; // single-room levels: list entries per working lane group of a refill
    int pregen_min;       // single-room levels: lane groups that work on a refill at least (k_pregen: entries / 32 otherwise); 0 = the whole grid, as mazes always get
    int pregen_group;     // lanes per env in k_pregen: 32 (two envs per wave), 16 or 64
    // the lane = level generator (bbai_genl.hpp, k_pregen_lane): every LevelGen parameterisation and the single-instruction levels without a lock-first prologue
    unsigned long long* tap_mask; uint32_t* tap_rank0; int32_t* tap_perm; int64_t* tap_ids; int64_t tap_count;     // bbai_step_tap_set: the envs bbai_step_tapped logs
    uint32_t* mtt;        // [n][2][MT_N] tempered outputs of the latest and the previous MT19937 generation of every env (NULL: kind not covered)
    uint8_t* mtpar;       // [n] which half holds the latest generation
    uint8_t* lane_tmpl;   // the kind's record template + C plane (lane_build_template)
    int lane_words;       // LDS words per lane (lane_layout)
    int pregen_lane;      // BBAI_PREGEN_LANE: 1 (default where covered) = k_pregen_lane generates, 0 = the lane-group kernel k_pregen
    int lane_blocks;      // upper bound on its waves per launch
    int step_prio;        // s_setprio level of the step-path kernels' waves (they share CUs with k_pregen)
    // optional per-kernel timing (bbai_profile): HIP event pairs on the launch stream around k_step / k_consume / k_render
    bool prof_on;
    struct ProfSlot { hipEvent_t a, b; bool used; } prof[3][PROF_RING];
    int prof_pos[3];
    double prof_ms[3];
    int64_t prof_n[3];
    int64_t prof_step_ticks;   // steps the bracketed k_step launches took (a bbai_rollout launch takes up to a window's worth): option "profile_step_ticks"
    int rollout_multi;    // bbai_rollout steps up to a look-ahead window per k_step launch (1, default) or one step per launch (0)
    int64_t tick;         // number of consume_and_refill calls so far
    uint8_t* vplane;      // [n][v_bytes] window plane (bbai_types.hpp): one 128-byte line per window-origin class; BBAI_VPLANE=0: none
    uint16_t* fcache;     // [n] appearance of the front cell (low byte) and of the carried object (high byte) after the last step
    uint8_t* cplane;      // [n][cpl_bytes] C plane rows of the small single rooms (bbai_types.hpp cpl_ok; in-place layout only); BBAI_CPLANE=0: none
    uint8_t* lsm;         // [n] done-action verifier mode only (BABYAI_DONE_ACTIONS / bbai_set_done_actions): bit k = leaf k's
                          //     lastStepMatch (babyai/levels/verifier.py:213-230); NULL = the normal mode
    unsigned int* render_tickets;   // [64][64] ticket counters of k_render_q + its departure counter (rows 0 .. 8), k_render_dstore_lw's (rows 32, 33); zero between launches (the kernels leave them so)
    int render_queue;     // -1 = by batch size (default), 0 = one-shot blocks only, m = queue shape m (render_launch)
    int render_queue_bpc; // persistent render blocks per CU (0 = 1024 threads' worth: ONE 1024-thread block per CU --
                          // profiles/r04/render_queue_ab_1M_b.jsonl: k_render 1.50 ms against 1.61 with two)
    int render_queue_blocks;   // their total number (0 = by render_queue_bpc)
    int render_pace;      // (experiment) 1/16 ns of wall clock per render ticket (then with two counters), 0 (default) = as fast as the
                          // one counter serves them
    // delta rendering: the registered 7x7-view buffer (bbai_set_render_target) and full-grid buffer (bbai_set_grid_target), each with the atlas tile ids of the frame it holds
    Targets targets;      // (bbai_target.hpp: the records, and the planner every frame-writing call asks -- frame_call)
    int rt_next_ts;       // "render_target_tile_size": the tile size the NEXT bbai_set_render_target registers (8, default)
    int render_delta;     // 1 (default) = renders into the registered buffer store only changed lines
    int render_delta_sched;    // k_render_delta: 0 (default) = interleaved groups per block, 1 = contiguous ranges, 2 as 0; the store-only render of pieces: 0 / 1 = the ticket queue (k_render_dstore_lw), 2 = the static split (k_render_dstore)
    int render_delta_tpb;      // 512 (default, also for 0) or 1024 threads per delta render block
    int render_delta_bpc;      // delta render blocks per CU (0 = the default: 3 of 512 threads, 1 of 1024; 1 of k_render_dstore_lw's 576)
    int render_piece_bytes;    // the delta render's store unit, 64-byte pieces (default) or 128 (whole lines)
    int render_delta_from_step;   // 1 = a step + render call finds the dirty cells in k_step, 0 = in the render, -1 (default) = by batch size
    int n_cus;            // compute units of the device
    int done_action_enum; // done-action mode only -- bbai_step's `done` actions count as the enum member (verifier.py:543-545)
    int reseed_levels;    // "reseed_levels": levels of the new stream a bbai_reseed generates per listed env (0 = the whole ring); the env parks behind them
    int step_hold;        // "step_hold": action byte BBAI_ACTION_HOLD means "this env sits the step out" under bbai_step / _render / _full / _tapped / bbai_rollout (0: it is `done`, as 8..255 are)
    int consume_fused;    // -1 = by batch size, 0 = k_consume launch, 1 = inside k_step
    int inplace;          // BBAI_INPLACE: the in-place layout (live_slot, bbai_kernels.hpp): an env's live record IS the look-ahead slot its episode was generated into
    uint8_t* atlas;       // [n_tiles][192]
    uint8_t* lut;         // [2][256]
    int n_tiles;
    uint8_t* grid_atlas[3];   // full-grid picture (bbai_set_grid_atlas), tile sizes 8 / 16 / 32: [GRID_MAX_TILES + 1][ts][ts][3]
    uint8_t* grid_lut[3];     // [2][5][256]
    int grid_tiles[3];        // installed tiles (0: none)
    int grid_bpc;             // "grid_render_bpc": k_render_grid blocks per CU (0 = by tile size)
    int grid_render_delta;    // 1 (default) = renders into the registered grid target store only the pieces that changed
    int grid_delta_group;     // "grid_delta_group": k_grid_delta envs per group (0 = by batch size; clamped to what its LDS planes hold: griddelta_shape)
    uint8_t* view_atlas[2];   // the 7x7 view's picture (bbai_set_view_atlas), tile sizes 16 / 32: [VIEWPX_MAX_TILES + 1][ts][ts][3]
    uint8_t* view_lut[2];     // [2][256]
    int view_tiles[2];        // installed tiles (0: none)
    uint8_t* vpx_atlas[3];    // the V x V view's picture (bbai_set_view_pixels_atlas), tile sizes 8 / 16 / 32: [VIEWPX_MAX_TILES + 1][ts][ts][3]
    uint8_t* vpx_lut[3];      // [2][256]
    int vpx_tiles[3];         // installed tiles (0: none)
    bool seeded, live;
    uint8_t* bot_state;   // [n][bot_state_bytes(bot_stack)] the expert's per-env plan (bbai_bot_act; allocated on first use)
    int bot_stack;        // subgoal stack capacity per env (BBAI_BOT_STACK, default 48)
    uint16_t* bot_work;   // [bot_threads][BOT_WORK_WORDS] BFS scratch per resident thread
    uint32_t* bot_rows;   // [bot_threads][2 * MAX_W] row masks of the second (through-blockers) search
    int bot_group;        // lanes per env of the expert kernel: 0 = lane = env (k_bot), 16 = one 16-lane group per env (k_botg)
    int bot_eager;        // BBAI_BOT_EAGER (default 1): expand the first search tree at the top of every decision
    int64_t bot_threads;
    uint64_t* bot_stats;  // [2] decisions that ended in a dead bot: by the reference's rules / by our capacity limits
    // bbai_reseed's scratch (reseed_scratch: allocated at the first call): a work list and sub-list counters shaped like gen_list / gen_count, a
    // `pending` / `first_slot` plane of its own, the envs a call has claimed (bbai_reseedk.hpp), and the events that order the call
    int32_t* rs_list;     // [SHARDS][gen_sublist_cap(n)]
    uint32_t* rs_count;   // [SHARDS][GEN_COUNT_U32]
    uint8_t* rs_pending;  // [n] zero between calls (the generator clears what it served)
    uint8_t* rs_first;    // [n] always zero: a reseeded ring is generated from slot 0
    uint32_t* rs_claim;   // [(n + 31) / 32] zero between calls
    hipEvent_t ev_rs_call, ev_rs_done, ev_rs_part[MAX_SIDES];
    Owner own;            // every allocation, pinned word, stream and event above (option "owned" counts them; bbai_destroy releases them)
};

#include "bbai_stepk.hpp"
#include "bbai_pregen.hpp"
#include "bbai_ring.hpp"
#include "bbai_botk.hpp"
#include "bbai_render.hpp"
#include "bbai_gridk.hpp"
#include "bbai_griddelta.hpp"
#include "bbai_viewn.hpp"
#include "bbai_viewpx.hpp"
#include "bbai_viewpxn.hpp"
#include "bbai_tokens.hpp"
#include "bbai_demo.hpp"
#include "bbai_statek.hpp"
#include "bbai_reseedk.hpp"


// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

int bbai_version(void) { return 200; }
const char* bbai_last_error(void) { return g_err; }

int bbai_fill_layout(bbai_level_cfg* cfg) {
    if (!cfg) ARG_FAIL("null cfg");
    LevelCfg c;
    memcpy(&c, cfg, sizeof(c));
    if (fill_layout(c) != 0) { snprintf(g_err, sizeof(g_err), "unsupported level geometry"); return BBAI_ERR_ARG; }
    memcpy(cfg, &c, sizeof(c));
    return BBAI_OK;
}

static int create_finish(bbai_env* e);

static int validate_cfg(const LevelCfg& c) {
    if (c.kind != K_GOTO && c.kind != K_LEVELGEN && c.kind != K_BONUS) return -1;
    if (c.kind == K_BONUS && (c.script < 1 || c.script >= BS_COUNT)) return -1;
    if (c.num_dists < 0) return -1;
    if (c.kind == K_GOTO) {
        if (!c.redball && c.num_dists < 1) return -1;
        if (c.instr < L_GOTO || c.instr > L_PUTNEXT || c.target < TG_REDBALL || c.target > TG_LOCKED_ROOM_OBJ) return -1;
        if (c.instr == L_PUTNEXT && (c.target != TG_TWO_DISTS || c.num_dists < 2)) return -1;
        if ((c.target == TG_LOCKED_DOOR || c.target == TG_LOCKED_ROOM_OBJ) != (c.lock != 0)) return -1;
        if (c.lock && c.num_rows * c.num_cols < 2) return -1;
    }
    if (c.kind == K_LEVELGEN) {
        if (c.n_action_kinds < 1 || c.n_action_kinds > 4 || c.n_instr_kinds < 1 || c.n_instr_kinds > 3) return -1;
        for (int i = 0; i < c.n_action_kinds; ++i) if (c.action_kinds[i] < 0 || c.action_kinds[i] > 3) return -1;
        for (int i = 0; i < c.n_instr_kinds; ++i) if (c.instr_kinds[i] < 0 || c.instr_kinds[i] > 2) return -1;
    }
    // max_steps must fit uint16: 8 navigations * S^2 * rows * cols
    if (8 * c.room_size * c.room_size * c.num_rows * c.num_cols > 65535) return -1;
    return 0;
}

static int inplace_by_default(const LevelCfg& c, int64_t n_envs) {
    // Measured, ms per step classic -> in-place, settings alternated in one process (tools/ab.py).  Round 4 (profiles/r04/inplace_*.jsonl): GoToLocal 32 768
    // envs 0.0253 -> 0.0183, 65 536 0.0341 -> 0.0322, PickupLoc 262 144 0.0780 -> 0.0733; mazes lose at every size (no window plane in this layout:
    // BossLevel 1 048 576 0.111 -> 0.133).  Round 5, after the list atomic left the step path (profiles/r05/inplace_size_sweep.jsonl): GoToLocal 262 144
    // 0.0832 -> 0.0720, GoToLocal 1 048 576 0.333 -> 0.305, PickupLoc 524 288 0.140 -> 0.127, PickupLoc 1 048 576 0.321 -> 0.331 (the one point where the
    // classic layout is ahead, by 3 %).  So: every single-room batch (the ring's own 64-GiB cap -- bbai_create -- bounds it; a ring that does not fit
    // falls back to a shorter look-ahead period, never to another layout).
    (void)n_envs;
    return c.num_rows * c.num_cols > 1 ? 0 : 1;
}

// bbai_create's steps, in the order it takes them (a failing one leaves the HIP error in g_hip).  Step 2: the layout (BBAI_INPLACE) and the per-env planes.
static int create_planes(bbai_env* e) {
    const LevelCfg& c = e->cfg; const size_t n = (size_t)e->n;
    BBAI_TRY(e->own.alloc({{&e->rec, n * c.rec_bytes, true},
                           {&e->hot, n * sizeof(Hot), true},       // (slot 0 before any seed: an in-place handle that is only imported into keeps its live records in slot depth - 1)
                           {&e->stale, n * 8}, {&e->mt, n * MT_N * 4}, {&e->mti, n * 4}, {&e->vhead, n * 4, true}, {&e->vset, n * 8 * 8, true},
                           {&e->pending, NWIN * n, true}, {&e->first_slot, NWIN * n, true}, {&e->win_meta, NWIN * META_U32 * 4, true},
                           {&e->totals, SHARDS * SHARD_U64 * 8, true}, {&e->flow, FLOW_WORDS * 8, true},
                           {&e->gen_list, (size_t)SHARDS * (size_t)gen_sublist_cap(e->n) * 4}, {&e->gen_count, SHARDS * GEN_COUNT_U32 * 4}}));
    e->gen_lists[0] = e->gen_list; e->gen_counts[0] = e->gen_count;         // (further look-ahead streams' lists: set_sides)
    // BBAI_INPLACE: 1 / 0 force the in-place layout (live_slot, bbai_kernels.hpp) on / off; default: by level family and batch size
    const char* iv = getenv("BBAI_INPLACE");
    e->inplace = iv ? (atoi(iv) != 0) : inplace_by_default(c, e->n);
    const char* vv = getenv("BBAI_VPLANE");              // 0: round 2's record-only step path (A/B runs)
    if (!(vv && atoi(vv) == 0) && !e->inplace) BBAI_TRY(e->own.alloc({{&e->vplane, n * v_bytes(c), true}, {&e->fcache, n * 2, true}}));
    const char* cv = getenv("BBAI_CPLANE");              // 0: the in-place step path of rounds 4-5 (window out of the record; A/B runs)
    if (e->inplace && cpl_ok(c) && !(cv && atoi(cv) == 0)) BBAI_TRY(e->own.alloc({{&e->cplane, n * cpl_bytes(c), true}, {&e->fcache, n * 2, true}}));
    return BBAI_OK;
}
// Step 3: the lane = level generator's state, where the kind and the layout are covered.
static int create_lane_gen(bbai_env* e) {
    const LevelCfg& c = e->cfg;
    if (!(lane_gen_ok(c) && (!e->inplace || cpl_ok(c)))) return BBAI_OK;
    // Default: the single rooms.  Measured (profiles/r06/NOTES.md): bulk fills 2.2 - 2.9 ns per level against 6 - 7 (PickupLoc 262 144: 0.057 -> 0.043 ms
    // per step); the mazes' bulk rates are 17 (GoTo) and 31 (BossLevel) ns against 30 and 20, and a maze refill of a few thousand levels
    // lasts milliseconds as ONE level per lane where the lane-group kernel needs a third of that -- the mazes keep k_pregen.
    const char* lv = getenv("BBAI_PREGEN_LANE");
    e->pregen_lane = lv ? (atoi(lv) != 0) : (c.num_rows * c.num_cols == 1);
    e->lane_words = lane_layout(c).words;
    std::vector<uint8_t> t((size_t)lane_template_bytes(c));
    BBAI_TRY(e->own.alloc({{&e->mtt, (size_t)e->n * 2 * MT_N * 4, true}, {&e->mtpar, (size_t)e->n, true}, {&e->lane_tmpl, t.size()}}));
    lane_build_template(c, t.data());
    HIP_TRY(hipMemcpy(e->lane_tmpl, t.data(), t.size(), hipMemcpyHostToDevice));
    return BBAI_OK;
}
// The look-ahead ring of one depth as temporaries: next_rec, next_hot and, in the in-place layout, next_obs -- all of them, or none and the sticky
// out-of-memory error cleared.  ring_install hands them to the handle, letting the ring it had go only now (bbai_checkpoint_load).
struct Ring { Scoped rec, hot, obs; };
static int ring_alloc(const bbai_env* e, int depth, Ring& r) {
    const size_t D = (size_t)depth, n = (size_t)e->n;
    int rc = r.rec.mem(D * n * e->cfg.rec_bytes);
    if (rc == BBAI_OK) rc = r.hot.mem(D * n * sizeof(Hot));
    if (rc == BBAI_OK && e->inplace) rc = r.obs.mem(D * n * OBS_SLOT);
    if (rc != BBAI_OK) { (void)hipGetLastError(); r.rec.reset(); r.hot.reset(); r.obs.reset(); }
    return rc;
}
static void ring_install(bbai_env* e, Ring& r, int period) {
    (void)e->own.drop(&e->next_rec); (void)e->own.drop(&e->next_hot); (void)e->own.drop(&e->next_obs);
    e->own.adopt(&e->next_rec, r.rec); e->own.adopt(&e->next_hot, r.hot); e->own.adopt(&e->next_obs, r.obs);
    e->period = period; e->depth = 2 * period + e->inplace;          // (in-place: the live slot + the 2B look-ahead levels)
}
// Step 4: the ring, at the longest period that fits.
static int create_ring(bbai_env* e) {
    const LevelCfg& c = e->cfg;
    // Refill period B (ticks per look-ahead refill, BBAI_LOOKAHEAD); ring depth D = 2B.  One k_pregen launch per
    // window lasts as long as its slowest level (hundreds of microseconds to milliseconds: rejection sampling has a
    // heavy tail) and has to land within one window, so B ticks of the step path must outlast it or the step stream
    // waits: default = the longest period of 96 (mazes), 64, 32, 16, 8, 4, 2 whose ring fits the cap.  (Up to 32 until round 6.  A refill launch lasts as
    // long as its slowest WAVE -- 0.4 ms for 64 single-room levels per lane-generator wave, 0.6-0.9 ms for a lane group's maze -- almost whatever its
    // size, and bbai_rollout's k_step takes 8 us per tick at 65 536 envs: 32 ticks no longer outlast a refill.  GoToLocal 65 536 envs 0.0146 -> 0.0103 ms
    // per step at 64, GoTo 131 072 0.0344 -> 0.0244 at 64 -> 0.0214 at 96: profiles/r06/NOTES.md section 9.)  The cap is BBAI_RING_GIB
    // (default 64 GiB -- the part has 288 GB; round 4: 1 048 576 GoTo envs waited for refills at period 4, the 16-GiB cap of
    // rounds 1-3) but never more than a quarter of the memory that is FREE right now (several handles or ranks
    // on one device, smaller parts), and an allocation that fails all the same is retried with half the period: a
    // shorter period only costs speed, never correctness.  (131072 GoTo envs -> 32; 1M BossLevel envs -> 16.)
    const char* ev = getenv("BBAI_LOOKAHEAD");
    const char* gv = getenv("BBAI_RING_GIB");
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = (size_t)64 << 30;
    const size_t slot_bytes = (size_t)e->n * c.rec_bytes;
    const size_t cap = std::min((size_t)(gv ? std::max(1, atoi(gv)) : 64) << 30, free_b / 4);
    int b = 2;
    if (ev) b = atoi(ev);
    else for (int cand : {96, 64, 32, 16, 8, 4, 2}) if (cand <= (c.num_rows * c.num_cols > 1 ? 96 : 64))      // (single rooms: 96 measured equal to 64)
         if (slot_bytes * (2 * (size_t)cand + (size_t)e->inplace) <= cap) { b = cand; break; }
    b = b < 1 ? 1 : (b > MAX_PERIOD ? MAX_PERIOD : b);
    for (;; b >>= 1) {
        Ring r;
        const int rc = ring_alloc(e, 2 * b + e->inplace, r);
        if (rc == BBAI_OK) {                           // (the ring that fits starts zeroed; next_hot is written by bbai_seed)
            ring_install(e, r, b);
            HIP_TRY(hipMemset(e->next_rec, 0, (size_t)e->depth * slot_bytes));
            if (e->next_obs) HIP_TRY(hipMemset(e->next_obs, 0, (size_t)e->depth * (size_t)e->n * OBS_SLOT));
            return BBAI_OK;
        }
        if (b == 1 || ev) return rc;                   // an explicit BBAI_LOOKAHEAD is a request, not a hint
    }
}

// Step 5: the small buffers.
static int create_small(bbai_env* e) {
    const size_t n = (size_t)e->n;
    // babyai/levels/verifier.py:17 `use_done_actions = os.environ.get('BABYAI_DONE_ACTIONS', False)`: any non-empty value
    const char* dv = getenv("BABYAI_DONE_ACTIONS");
    if (dv && dv[0]) BBAI_TRY(e->own.alloc({{&e->lsm, n, true}}));
    return e->own.alloc({{&e->reset_list, n * 4}, {&e->reset_slot, n}, {&e->counters, 128, true}, {&e->atlas, MAX_TILES * TILE_BYTES},
                         {&e->render_tickets, 64 * 64 * 4, true}, {&e->lut, 512}});
}
// Step 6: the pinned flag words, zeroed, and the device's address of them.
static int create_pinned(bbai_env* e) {
    Scoped hf;
    void* dv = nullptr;
    BBAI_TRY(hf.pinned(64));
    memset(hf.h, 0, 64);
    e->own.adopt(&e->host_flags, hf);
    HIP_TRY(hipHostGetDevicePointer(&dv, (void*)e->host_flags, 0));
    e->host_flags_dev = (uint32_t*)dv;
    return BBAI_OK;
}

int bbai_create(const bbai_level_cfg* cfg, int64_t n_envs, int device, bbai_env** out) {
    if (!cfg || !out || n_envs <= 0 || n_envs > (1ll << 30)) { snprintf(g_err, sizeof(g_err), "bad argument"); return BBAI_ERR_ARG; }
    LevelCfg c;
    memcpy(&c, cfg, sizeof(c));
    LevelCfg chk = c;
    if (fill_layout(chk) != 0 || memcmp(&chk, &c, sizeof(c)) != 0 || validate_cfg(c) != 0) {
        snprintf(g_err, sizeof(g_err), "level configuration rejected (layout not filled or out of range)");
        return BBAI_ERR_ARG;
    }
    ON_DEVICE(device);
    bbai_env* e = new bbai_env();          // (value-initialised: every field starts zero)
    e->cfg = c; e->n = n_envs; e->device = device;
    int rc = BBAI_OK;
    for (auto step : {create_planes, create_lane_gen, create_ring, create_small, create_pinned}) if (rc == BBAI_OK) rc = step(e);
    if (rc != BBAI_OK) {
        snprintf(g_err, sizeof(g_err), "hipMalloc failed: %s", hipGetErrorString(g_hip));
        bbai_destroy(e);
        return BBAI_ERR_NOMEM;
    }
    if ((rc = create_finish(e)) != BBAI_OK) { bbai_destroy(e); return rc; }      // g_err holds the failing call
    *out = e;
    return BBAI_OK;
}

}  // extern "C"

// The performance knobs (include/bbai.h: bbai_set_option), one row each: the option's name, the BBAI_* variable bbai_create reads (or none), the
// field, the default, and how a raw value -- from the variable or from bbai_set_option alike -- becomes the stored one.  The read-only rows
// at the end are looked up by bbai_get_option alone (their fields are set elsewhere).  Never semantics: every setting produces the same bytes --
// but for the three semantic switches that ride in this table because the C surface is closed: "done_action_enum", "reseed_levels" and "step_hold".
enum KnobNorm { AS_IS, FLAG /* v != 0 */, AT_LEAST /* max(lo, v) */, TRI /* v < 0: -1, else v != 0 */ };
struct Knob { const char* name; const char* var; int bbai_env::*field; int def; KnobNorm norm; int lo; bool read_only; };
static const Knob KNOBS[] = {
    {"render_queue", "BBAI_RENDER_QUEUE", &bbai_env::render_queue, -1},
    {"render_queue_bpc", nullptr, &bbai_env::render_queue_bpc, 0},
    {"render_queue_blocks", nullptr, &bbai_env::render_queue_blocks, 0},
    {"render_pace", "BBAI_RENDER_PACE", &bbai_env::render_pace, 0, AT_LEAST, 0},
    {"render_group", "BBAI_RENDER_GROUP", &bbai_env::render_group, 0},
    {"render_tpb", "BBAI_RENDER_TPB", &bbai_env::render_tpb, 0},
    {"render_delta", "BBAI_RENDER_DELTA", &bbai_env::render_delta, 1, FLAG},                  // (a set also drops the shadow)
    {"render_delta_sched", nullptr, &bbai_env::render_delta_sched, 0},
    {"render_delta_tpb", nullptr, &bbai_env::render_delta_tpb, 0},
    {"render_delta_bpc", nullptr, &bbai_env::render_delta_bpc, 0, AT_LEAST, 0},
    {"render_delta_from_step", nullptr, &bbai_env::render_delta_from_step, -1, TRI},
    {"render_piece_bytes", nullptr, &bbai_env::render_piece_bytes, RENDER_PIECE_DEFAULT},   // (64 or 128: bbai_set_option refuses the rest)
    {"render_target_tile_size", nullptr, &bbai_env::rt_next_ts, TILE},                        // (8, 16 or 32: bbai_set_option refuses the rest)
    {"grid_render_bpc", nullptr, &bbai_env::grid_bpc, 0, AT_LEAST, 0},
    {"grid_render_delta", nullptr, &bbai_env::grid_render_delta, 1, FLAG},                    // (0: whole frames, the shadow kept behind them)
    {"grid_delta_group", nullptr, &bbai_env::grid_delta_group, 0, AT_LEAST, 0},
    {"step_prio", "BBAI_STEP_PRIO", &bbai_env::step_prio, 1},                          // (never slower, GoTo 131 072 envs -2 %: profiles/r03/step_prio_ab.jsonl)
    {"pregen_group", "BBAI_PREGEN_GROUP", &bbai_env::pregen_group, 32},
    // lane groups of a refill launch at most: 16 384 = two generator waves per SIMD of the part, the other half of every SIMD stays with the step
    // kernels (profiles/r05/pregen_residency_cap_ab.jsonl, ms per step at 32 768 / 16 384 / 8 192 / 4 096 groups: GoTo 131 072 envs 0.0438 / 0.0390 /
    // 0.0395 / 0.0478; BossLevel encoded 1 048 576 0.110 / 0.104 / 0.104; BossLevel pixels 131 072: no difference).  bbai_seed's first fill
    // (nothing else runs) takes the whole part: 32 768.
    {"pregen_blocks", "BBAI_PREGEN_BLOCKS", &bbai_env::pregen_cap, 16384, AT_LEAST, 64},
    {"pregen_min", "BBAI_PREGEN_MIN", &bbai_env::pregen_min, 6144, AT_LEAST, 0},
    {"pregen_per_group", "BBAI_PREGEN_PER_GROUP", &bbai_env::pregen_per_group, 12, AT_LEAST, 1},
    {"lane_blocks", "BBAI_LANE_BLOCKS", &bbai_env::lane_blocks, 16384, AT_LEAST, 1},            // (0 on a handle without the lane generator: create_finish)
    {"consume_fused", "BBAI_CONSUME_FUSED", &bbai_env::consume_fused, -1},
    {"gate_strict", "BBAI_GATE_STRICT", &bbai_env::gate_strict, 0, FLAG},
    {"gate_probe", "BBAI_GATE_PROBE", &bbai_env::gate_probe, 1},                       // (a set also forgets the verdicts)
    {"bot_group", "BBAI_BOT_GROUP", &bbai_env::bot_group, 0},
    {"step_render_split", "BBAI_STEP_RENDER_SPLIT", &bbai_env::step_render_split, -1},
    {"rollout_multi", "BBAI_ROLLOUT_MULTI", &bbai_env::rollout_multi, 1},
    {"done_action_enum", nullptr, &bbai_env::done_action_enum, 0, FLAG},                      // (a SEMANTIC switch, the first of three in this list: include/bbai.h bbai_set_done_actions)
    {"reseed_levels", nullptr, &bbai_env::reseed_levels, 0, AT_LEAST, 0},                     // (the second SEMANTIC switch: the depth of the next bbai_reseed calls; a host value read when a call is enqueued)
    {"step_hold", nullptr, &bbai_env::step_hold, 0, FLAG},                                    // (the third SEMANTIC switch: BBAI_ACTION_HOLD; like "reseed_levels" a host value read when a stepping call is enqueued)
    {"pregen_lane", nullptr, &bbai_env::pregen_lane, 0, AS_IS, 0, true},                              // (set: bbai_set_option converts the generator state)
    {"lookahead_streams", nullptr, &bbai_env::n_sides, 0, AS_IS, 0, true},                            // (set: set_sides)
    {"gate_forced_strict", nullptr, &bbai_env::gate_forced, 0, AS_IS, 0, true},                       // 1: the caller's stream failed the concurrency probe
    {"inplace", nullptr, &bbai_env::inplace, 0, AS_IS, 0, true},
    {"lookahead_period", nullptr, &bbai_env::period, 0, AS_IS, 0, true},                              // the refill period the handle chose
};
static const Knob* find_knob(const char* name) {
    for (const Knob& k : KNOBS) if (!strcmp(name, k.name)) return &k;
    return nullptr;
}
static int knob_value(const Knob& k, int v) {
    return k.norm == FLAG ? v != 0 : k.norm == AT_LEAST ? std::max(k.lo, v) : k.norm == TRI ? (v < 0 ? -1 : v != 0) : v;
}

// The look-ahead streams beyond the first, and the stream k_mark needs once there are several, exist only while asked for: every HIP stream
// is a hardware queue, and a dozen of them made EVERY dispatch of a handle that used two wait its turn (k_step 10 -> 50 us whenever a refill ran,
// profiles/r06/NOTES.md section 9).
static int set_sides(bbai_env* e, int want) {
    want = std::max(1, std::min(MAX_SIDES, want));
    Owner& o = e->own;
    Scoped side[MAX_SIDES], list[MAX_SIDES], count[MAX_SIDES], mark, part[MAX_SIDES];       // going up: whatever is missing (a lower setting leaves lists and events behind), all of it or none
    for (int k = 1; k < want; ++k) {
        if (!e->sides[k]) BBAI_TRY(side[k].stream(hipStreamNonBlocking, &e->side_prio));
        if (!e->gen_lists[k]) BBAI_TRY(list[k].mem((size_t)SHARDS * (size_t)gen_sublist_cap(e->n) * 4));
        if (!e->gen_counts[k]) BBAI_TRY(count[k].mem(SHARDS * GEN_COUNT_U32 * 4));
    }
    if (want > 1 && !e->mark_stream) BBAI_TRY(mark.stream(hipStreamNonBlocking, &e->side_prio));
    for (int k = 0; k < want && want > 1; ++k) if (!e->ev_part[k]) BBAI_TRY(part[k].event());
    for (int k = 0; k < want; ++k) { o.adopt(&e->sides[k], side[k]); o.adopt(&e->gen_lists[k], list[k]); o.adopt(&e->gen_counts[k], count[k]); o.adopt(&e->ev_part[k], part[k]); }
    o.adopt(&e->mark_stream, mark);
    for (int k = std::max(1, want); k < MAX_SIDES; ++k) BBAI_TRY(o.drop(&e->sides[k]));      // going down: the streams go, their lists and events stay
    if (want == 1) BBAI_TRY(o.drop(&e->mark_stream));
    e->n_sides = want;
    e->n_probed = 0;
    return BBAI_OK;
}
static int create_finish(bbai_env* e) {
    if (hipDeviceGetAttribute(&e->n_cus, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess) e->n_cus = 0;
    // The look-ahead stream.  (Confining it to a subset of the CUs with a CU mask was measured in round 3 --
    // profiles/r03/pregen_cus_ab.jsonl: 32 / 64 / 96 / 128 CUs change no step time by more than 1 %, and a masked stream is a
    // BLOCKING stream: with a caller on the NULL stream it serialises generation and stepping, 46 -> 72 us per step at
    // 65 536 GoToLocal envs.  Not kept.  Round 6 tried again for callers on their own stream: on this pool's runtime
    // hipExtStreamCreateWithCUMask changes NOTHING -- a bulk fill confined to 32 of 256 CUs runs at the unconfined rate
    // (profiles/r06/NOTES.md section 6).)
    int lo = 0, hi = 0;     // look-ahead generation should get wave slots as soon as any free up
    HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    const char* pv = getenv("BBAI_PREGEN_PRIORITY");     // 1 (default): highest priority, 0: default priority
    e->side_prio = (pv && atoi(pv) == 0) ? lo : hi;
    BBAI_TRY(e->own.stream(&e->side, hipStreamNonBlocking, &e->side_prio));
    e->sides[0] = e->side;
    const char* ls = getenv("BBAI_LOOKAHEAD_STREAMS");
    BBAI_TRY(set_sides(e, ls ? atoi(ls) : LOOKAHEAD_STREAMS_DEFAULT));
    BBAI_TRY(e->own.event(&e->ev_consumed));
    BBAI_TRY(e->own.stream(&e->split, hipStreamNonBlocking));
    BBAI_TRY(e->own.event(&e->ev_split0));
    BBAI_TRY(e->own.event(&e->ev_splitB));
    for (int k = 0; k < NWIN; ++k) BBAI_TRY(e->own.event(&e->ev_refill[k]));
    BBAI_TRY(e->own.event(&e->ev_switch));
    const char* cv = getenv("BBAI_CALL_EVENTS");
    e->call_events = cv && atoi(cv) != 0;
    for (const Knob& k : KNOBS) if (!k.read_only) {
        const char* kv = k.var ? getenv(k.var) : nullptr;
        e->*k.field = kv ? knob_value(k, atoi(kv)) : k.def;
    }
    if (!e->mtt) e->lane_blocks = 0;        // (no lane generator on this handle)
    return BBAI_OK;
}

extern "C" {

void bbai_destroy(bbai_env* e) {
    if (!e) return;
    DeviceGuard guard_(e->device);
    (void)hipDeviceSynchronize();
    e->own.drop_all();
    delete e;
}

}  // extern "C"

// k_pregen is instantiated per level family so that a launch carries only that family's mission code, and per group
// width G (envs per wave = 64 / G; BBAI_PREGEN_GROUP, default 32: two envs per wave)
template <int G>
static void launch_pregen_g(const bbai_env* e, unsigned groups, bool listed /* false: dense -- every env, the whole grid works */, uint8_t* pending, const uint8_t* first_slot, int side,
                            const int32_t* list /* NULL: the side's own work list and counters (a window's refill) */, const uint32_t* list_count) {
    unsigned long long* fails = e->flow + FLOW_GEN_FAILURES;
    const dim3 g((groups + 64 / G - 1) / (64 / G)), b(64);
    // Demand-sized groups only where a level is cheap (single rooms, <= 60 us per group): a maze level costs a group ~300 us,
    // and GoTo at 131 072 envs stalls the step stream with 4 entries per group (0.0534 vs 0.0385 ms per step,
    // profiles/r04/pregen_min_ab.jsonl) -- mazes keep the whole grid.
    const int min_groups = e->cfg.num_rows * e->cfg.num_cols > 1 ? 0 : e->pregen_min;
#define PREGEN_LAUNCH(KK, OO) hipLaunchKernelGGL((k_pregen<KK, G, OO>), g, b, 0, e->sides[side], e->cfg, e->n, e->next_rec, e->next_hot, e->mt, e->mti, list ? list : e->gen_lists[side], \
                                                listed ? (list ? list_count : e->gen_counts[side]) : nullptr, e->depth, pending, first_slot, fails, min_groups, e->pregen_per_group, e->next_obs)
    if (e->cfg.kind == K_LEVELGEN) { if (e->next_obs) PREGEN_LAUNCH(K_LEVELGEN, true); else PREGEN_LAUNCH(K_LEVELGEN, false); }
    else if (e->cfg.kind == K_BONUS) { if (e->next_obs) PREGEN_LAUNCH(K_BONUS, true); else PREGEN_LAUNCH(K_BONUS, false); }
    else { if (e->next_obs) PREGEN_LAUNCH(K_GOTO, true); else PREGEN_LAUNCH(K_GOTO, false); }
#undef PREGEN_LAUNCH
}
// k_pregen_lane lives in a translation unit of its own (bbai_genlane.hip: compiled without machine-CSE, see there)
static void launch_pregen_lane(const bbai_env* e, int64_t entries_hint, bool listed, uint8_t* pending, const uint8_t* first_slot, int side,
                               const int32_t* list, const uint32_t* list_count) {
    LaneLaunch a;
    a.cfg = e->cfg; a.n = e->n; a.next_rec = e->next_rec; a.next_hot = e->next_hot; a.mt = e->mt; a.mtt = e->mtt; a.mtpar = e->mtpar; a.mti = e->mti;
    a.gen_list = list ? list : e->gen_lists[side]; a.gen_count = listed ? (list ? list_count : e->gen_counts[side]) : nullptr; a.depth = e->depth; a.pending = pending; a.first_slot = first_slot;
    a.fails = e->flow + FLOW_GEN_FAILURES; a.next_obs = e->next_obs; a.tmpl = e->lane_tmpl; a.lane_words = e->lane_words;
    a.blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((entries_hint + 63) / 64, e->lane_blocks));
    a.stream = e->sides[side];
    bbai_lane_launch(a);
}
static void launch_pregen(const bbai_env* e, unsigned groups, bool listed, uint8_t* pending, const uint8_t* first_slot, int64_t entries_hint, int side = 0,
                          const int32_t* list = nullptr /* bbai_reseed: its own work list and counters instead of the side's */, const uint32_t* list_count = nullptr) {
    if (e->pregen_lane) { launch_pregen_lane(e, entries_hint, listed, pending, first_slot, side, list, list_count); return; }
    // Measured (profiles/r03/gen_rate_by_group_width.jsonl, pregen_group_width_in_bench.jsonl): levels per second of a bulk
    // fill 64 -> 32 -> 16 lanes per env: BossLevel 1 : 1.16 : 1.18, GoTo 1 : 1.13 : 1.17, PickupLoc 1 : 1.20 : 1.27,
    // GoToLocal 1 : 1.25 : 1.36; inside the step loop 32 is never behind 64 (GoToLocal 65 536 envs -3 %, PickupLoc 262 144
    // -6 %, GoTo 131 072 +-0) while 16 costs the step kernels of GoTo 131 072 9 % (fewer, fatter generator waves next to
    // them: 200 VGPRs and 20 KB of LDS each).
    if (e->pregen_group == 64) launch_pregen_g<64>(e, groups, listed, pending, first_slot, side, list, list_count);
    else if (e->pregen_group == 16) launch_pregen_g<16>(e, groups, listed, pending, first_slot, side, list, list_count);
    else launch_pregen_g<32>(e, groups, listed, pending, first_slot, side, list, list_count);
}

extern "C" {

static unsigned pregen_grid(const bbai_env* e, int64_t count_hint) {
    // one lane group per env, capped at pregen_cap groups in flight (the rest is reached by the groups' strides)
    int64_t g = std::min<int64_t>(count_hint, e->pregen_cap);
    return (unsigned)std::max<int64_t>(g, 1);
}

// A handle's launches are ordered by ONE caller stream at a time (plus the private look-ahead stream, which is tied to
// it by events).  A call that arrives on a DIFFERENT stream than the previous one is ordered behind everything the
// handle enqueued before.  Two ways to get the event that stream waits for (bbai_set_call_events):
//   off (default)  the event is recorded on the PREVIOUS stream at the moment of the switch -- free on the step path, but
//                  the previous stream must still exist then;
//   on             every call ends by recording the handle's completion event on its own stream and a switch only waits
//                  for it: the previous stream is never touched again (it may have been destroyed).  Measured cost
//                  (profiles/r03/call_events_ab.jsonl): +3.4 us per step at 65 536 GoToLocal envs (46.9 vs 43.5 us), +7 us
//                  per step + render at 131 072 pixel envs -- which is why it is opt-in.
static int enter_call(bbai_env* e, hipStream_t s) {
    if (e->host_flags && e->host_flags[0]) {         // (a plain read of pinned host memory: nothing is synchronised)
        snprintf(g_err, sizeof(g_err), "a window gate of this handle timed out waiting for a look-ahead refill (k_gate): its state is void -- "
                                       "re-seed it (bbai_seed) or destroy it");
        return BBAI_ERR_STATE;
    }
    if (e->have_stream && e->last_stream != s) {
        if (!e->call_events) HIP_TRY(hipEventRecord(e->ev_switch, e->last_stream));
        HIP_TRY(hipStreamWaitEvent(s, e->ev_switch, 0));
    }
    e->last_stream = s;
    e->have_stream = true;
    return BBAI_OK;
}
static int leave_call(bbai_env* e, hipStream_t s) {
    if (e->call_events) HIP_TRY(hipEventRecord(e->ev_switch, s));
    return BBAI_OK;
}
// enter_call / leave_call as a scope: once a call has entered, EVERY exit path -- also the error returns after work was
// already enqueued -- records the handle's completion event (call_events mode), so that a later call on another stream
// never waits for less than the handle really enqueued.  `return scope.leave();` on the success path reports a failing
// event record; the destructor covers the others.
struct CallScope {
    bbai_env* e; hipStream_t s; int rc; bool open;
    CallScope(bbai_env* e_, hipStream_t s_) : e(e_), s(s_), rc(enter_call(e_, s_)), open(false) { open = rc == BBAI_OK; }
    int leave() { open = false; return leave_call(e, s); }
    ~CallScope() { if (open) (void)leave_call(e, s); }
    CallScope(const CallScope&) = delete;
    CallScope& operator=(const CallScope&) = delete;
};

// bbai_profile: bracket a launch with an event pair (ring of PROF_RING pairs per kernel; a pair is folded into the sums
// when its slot comes round again, i.e. long after it completed, or when the totals are read)
static void prof_fold(bbai_env* e, int k, int i) {
    bbai_env::ProfSlot& p = e->prof[k][i];
    if (!p.used) return;
    float ms = 0;
    if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { e->prof_ms[k] += ms; e->prof_n[k]++; }
    p.used = false;
}
struct ProfScope {
    bbai_env* e; int k; hipStream_t s; int i;
    ProfScope(bbai_env* e_, int k_, hipStream_t s_) : e(e_), k(k_), s(s_), i(-1) {
        if (!e->prof_on) return;
        i = e->prof_pos[k];
        e->prof_pos[k] = (i + 1) % PROF_RING;
        prof_fold(e, k, i);
        if (!e->prof[k][i].a) { (void)e->own.event(&e->prof[k][i].a, hipEventDefault); (void)e->own.event(&e->prof[k][i].b, hipEventDefault); }
        (void)hipEventRecord(e->prof[k][i].a, s);
    }
    ~ProfScope() {
        if (i < 0) return;
        (void)hipEventRecord(e->prof[k][i].b, s);
        e->prof[k][i].used = true;
    }
};

// A consume-tick (one reset() or one auto-resetting step) in three parts: window_begin -- at the first tick of a window k_gate holds
// the stream until every env is sure to find B ready levels (NWIN, bbai_kernels.hpp); the consume itself -- k_consume over the reset list,
// or, fused, inside k_step (which therefore has to be launched AFTER window_begin); window_end -- the mission tokens of the new
// episodes and, at the last tick of a window, the window's close and ONE refill launch on the look-ahead stream for everything it consumed.
struct TickPos { int wb, pos; };
static TickPos tick_pos(const bbai_env* e) {
    const int64_t w = e->tick / e->period;           // window of this consume-tick
    return {(int)(w % NWIN), (int)(e->tick % e->period)};      // its buffer (pending / first_slot / meta), its place in the window
}
// Do kernels of stream `s` and of the look-ahead stream run concurrently?  Asked once per caller stream, at the first window it opens (a handle
// follows one stream at a time; up to 8 are remembered, a ninth is simply probed again).  Costs one stream synchronisation.
static int probe_stream(bbai_env* e, hipStream_t s, bool* ok) {
    for (int k = 0; k < e->n_probed; ++k) if (e->probed[k] == s) { *ok = e->probed_ok[k]; return BBAI_OK; }
    bool verdict = true;
    if (e->gate_probe == 2) verdict = false;
    else if (e->gate_probe != 0) {
        e->host_flags[1] = 0;
        hipLaunchKernelGGL(k_probe_set, dim3(1), dim3(1), 0, s, e->flow, 0ull);
        hipLaunchKernelGGL(k_probe_wait, dim3(1), dim3(1), 0, s, e->flow, e->host_flags_dev + 1);
        // (the releasing kernel sits behind an event of EVERY look-ahead stream, on the stream k_mark uses: all of them have to run beside the caller's)
        for (int k = 0; k < e->n_sides && e->n_sides > 1; ++k) {
            hipLaunchKernelGGL(k_probe_set, dim3(1), dim3(1), 0, e->sides[k], e->flow, 0ull);
            HIP_TRY(hipEventRecord(e->ev_part[k], e->sides[k]));
            HIP_TRY(hipStreamWaitEvent(e->mark_stream, e->ev_part[k], 0));
        }
        hipLaunchKernelGGL(k_probe_set, dim3(1), dim3(1), 0, e->n_sides > 1 ? e->mark_stream : e->side, e->flow, 1ull);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        verdict = e->host_flags[1] == 1;
    }
    const int at = e->n_probed < 8 ? e->n_probed++ : 7;
    e->probed[at] = s; e->probed_ok[at] = verdict;
    *ok = verdict;
    return BBAI_OK;
}
static int window_begin(bbai_env* e, hipStream_t s) {
    if (e->tick % e->period == 0) {
        const int64_t x = e->tick / e->period;
        bool strict = e->gate_strict != 0;
        if (!strict) {
            bool ok = true;
            BBAI_TRY(probe_stream(e, s, &ok));
            e->gate_forced = ok ? 0 : 1;
            strict = !ok;
        }
        if (strict && x >= 2) HIP_TRY(hipStreamWaitEvent(s, e->ev_refill[(x - 2) % NWIN], 0));
        hipLaunchKernelGGL(k_gate, dim3(1), dim3(64), 0, s, e->flow, e->win_meta, (unsigned long long)(e->tick / e->period), e->period, e->host_flags_dev);
        HIP_TRY(hipGetLastError());
    }
    return BBAI_OK;
}
static int window_end(bbai_env* e, hipStream_t s, int tokens_mode /* k_tokens: 0 list, 1 every env, 2 by `dones` */, const uint8_t* dones,
                      int ticks = 1 /* consume-ticks the launch in front took (bbai_rollout: up to the window's last; no token buffer then) */) {
    const int B = e->period;
    const TickPos tp = tick_pos(e);
    const int wb = tp.wb, pos = tp.pos + ticks - 1;         // (the launch's LAST tick: all of them lie in this window)
    if (e->tokens) {
        const int64_t hint = tokens_mode ? e->n : std::max<int64_t>(e->n / 64, 64);
        hipLaunchKernelGGL(k_tokens, dim3((unsigned)std::min<int64_t>((hint + 63) / 64, 4096)), dim3(64), 0, s, e->cfg, e->n, e->rec, e->inplace ? e->next_rec : nullptr, e->depth, e->hot,
                           e->tokens, e->reset_list, e->counters + 16 * e->step_parity, tokens_mode, dones);
    }
    if (tokens_mode == 0) {                  // (unfused: the ping-pong list counters)
        e->step_parity ^= 1;
        e->next_counter_clean = true;
    }
    HIP_TRY(hipGetLastError());
    if (pos == B - 1) {
        // Window end, on the look-ahead stream: the window's work list (k_compact), one refill launch for everything consumed in it, the mark behind it.
        const int64_t w = e->tick / B;
        HIP_TRY(hipEventRecord(e->ev_consumed, s));
        const int64_t nb = (e->n + 63) / 64;
        const int S = (int)std::max<int64_t>(1, std::min<int64_t>(e->n_sides, nb / 4));          // (a stream's range: at least 256 envs; the streams beyond S idle)
        for (int k = 0; k < S; ++k) {
            const int64_t w0 = nb * k / S, w1 = nb * (k + 1) / S, ne = std::min<int64_t>(e->n, w1 * 64) - w0 * 64;
            hipStream_t ss = e->sides[k];
            HIP_TRY(hipStreamWaitEvent(ss, e->ev_consumed, 0));
            HIP_TRY(hipMemsetAsync(e->gen_counts[k], 0, SHARDS * GEN_COUNT_U32 * 4, ss));
            hipLaunchKernelGGL(k_compact, dim3((unsigned)((w1 - w0 + 3) / 4)), dim3(256), 0, ss, e->n, e->pending + (size_t)wb * e->n, e->gen_lists[k], e->gen_counts[k], w0, w1 - w0);
            const int64_t rh = std::max<int64_t>((int64_t)B * (ne / 64), 64);
            launch_pregen(e, (unsigned)std::max<int64_t>(1, std::min<int64_t>(rh, e->pregen_cap / S)), true, e->pending + (size_t)wb * e->n, e->first_slot + (size_t)wb * e->n,
                          std::min<int64_t>(ne, 2 * rh), k);
            if (e->n_sides > 1) {
                HIP_TRY(hipEventRecord(e->ev_part[k], ss));
                HIP_TRY(hipStreamWaitEvent(e->mark_stream, e->ev_part[k], 0));
            }
        }
        hipStream_t ms = e->n_sides > 1 ? e->mark_stream : e->side;
        hipLaunchKernelGGL(k_mark, dim3(1), dim3(1), 0, ms, e->flow, (unsigned long long)(w + 1));
        HIP_TRY(hipEventRecord(e->ev_refill[wb], ms));
        HIP_TRY(hipGetLastError());
    }
    e->tick += ticks;
    return BBAI_OK;
}
// main stream: slots -> live state (+ first obs) by k_consume; side stream: refill the consumed slots.
static int consume_and_refill(bbai_env* e, hipStream_t s, uint8_t* image, uint8_t* dirs, int all) {
    BBAI_TRY(window_begin(e, s));
    const TickPos tp = tick_pos(e);
    const int wb = tp.wb;
    const int64_t hint = all ? e->n : std::max<int64_t>(e->n / 64, 64);
    {
    ProfScope prof_(e, 1, s);
    hipLaunchKernelGGL(k_consume, dim3((unsigned)std::min<int64_t>((hint + 3) / 4, 8192)), dim3(256), 0, s, e->cfg, e->n, e->rec,
                       e->hot, e->stale, e->next_rec, e->next_hot, e->vhead, e->vset, e->reset_list, e->reset_slot, e->counters + 16 * e->step_parity, all,
                       e->totals, e->depth, e->pending + (size_t)wb * e->n, e->first_slot + (size_t)wb * e->n,
                       e->win_meta + (size_t)wb * META_U32, image, dirs,
                       e->counters + 16 * (e->step_parity ^ 1), e->step_prio, e->vplane, e->fcache, e->lsm, e->inplace, e->cplane);
    }
    return window_end(e, s, all ? 1 : 0, nullptr);
}

int bbai_seed(bbai_env* e, const uint64_t* seeds, int64_t n) {
    if (!e || !seeds || n != e->n) { snprintf(g_err, sizeof(g_err), "seed: need exactly n_envs seeds"); return BBAI_ERR_ARG; }
    ON_DEVICE(e->device);
    HIP_TRY(hipDeviceSynchronize());             // nothing of an earlier run may still be in flight on either stream
    // 8 bytes per env cross PCIe; sha512 + init_by_array run per lane (k_seed).  Staged in a buffer of its own (parked in the
    // verifier's obj_set area, a re-seed of a live handle followed by a hot-only import left every env's verifier sets zeroed).
    Scoped staged;
    BBAI_TRY(staged.mem((size_t)n * 8));
    uint64_t* const seeds_dev = (uint64_t*)staged.h;
    HIP_TRY(hipMemcpy(seeds_dev, seeds, (size_t)n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_seed, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, e->side, n, seeds_dev, e->mt, e->mti);
    hipLaunchKernelGGL(k_init_hot, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->side, n, e->hot, e->next_hot, e->stale, e->depth);
    // fill every env's look-ahead ring with the first D levels of its stream (slot order == stream order).  EVERY
    // window buffer starts clean: a re-seed may land in the middle of a window that was using any of them.
    HIP_TRY(hipMemsetAsync(e->pending, 0, NWIN * (size_t)n, e->side));
    HIP_TRY(hipMemsetAsync(e->first_slot, 0, NWIN * (size_t)n, e->side));
    HIP_TRY(hipMemsetAsync(e->pending, e->depth - e->inplace, (size_t)n, e->side));      // (in-place: slot depth - 1 is the live one -- empty until the first reset)
    if (e->mtpar) HIP_TRY(hipMemsetAsync(e->mtpar, 0, (size_t)n, e->side));      // (position 624 of generation 0: the first draw's twist fills the other half)
    launch_pregen(e, (unsigned)std::max<int64_t>(1, std::min<int64_t>(n, std::max(e->pregen_cap, 32768))), false, e->pending, e->first_slot, n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(e->win_meta, 0, NWIN * META_U32 * 4, e->side));
    HIP_TRY(hipMemsetAsync(e->counters, 0, 128, e->side));
    {   // the refill count starts over (window numbering restarts with tick 0); the reset total, the give-up and the time-out counts keep running
        HIP_TRY(hipDeviceSynchronize());
        const unsigned long long zero = 0;
        HIP_TRY(hipMemcpy(e->flow + FLOW_REFILLED, &zero, 8, hipMemcpyHostToDevice));
    }
    for (int k = 0; k < NWIN; ++k) HIP_TRY(hipEventRecord(e->ev_refill[k], e->side));
    e->tick = 0;
    e->step_parity = 0;
    e->next_counter_clean = true;
    HIP_TRY(hipDeviceSynchronize());
    e->host_flags[0] = 0;            // every ring slot was just regenerated: a handle voided by a gate time-out is whole again
    e->seeded = true;
    e->live = false;
    return BBAI_OK;
}

int bbai_reset(bbai_env* e, uint8_t* image, uint8_t* dirs, void* stream) {
    if (!e || !image || !dirs) ARG_FAIL("null handle or output buffer");
    if (!e->seeded) { snprintf(g_err, sizeof(g_err), "reset before seed"); return BBAI_ERR_STATE; }
    ON_DEVICE(e->device);
    hipStream_t s = (hipStream_t)stream;
    CallScope call(e, s);
    BBAI_TRY(call.rc);
    BBAI_TRY(consume_and_refill(e, s, image, dirs, 1));
    e->live = true;
    return call.leave();
}

// k_step (+ the consume / refill of the envs it finished) on stream s; the caller has entered the call
static bool use_fused_consume(const bbai_env* e) {
    // option "consume_fused" / BBAI_CONSUME_FUSED: 1 = the stepping wave consumes its finished envs itself, 0 = k_consume launch,
    // -1 (default) = by level family.
    if (e->consume_fused >= 0) return e->consume_fused != 0;
    // Measured (profiles/r04/consume_fused_ab.jsonl, ms per step unfused -> fused): the mazes win -- GoTo 131 072 envs 0.046 -> 0.041,
    // GoTo 1 048 576 0.245 -> 0.211, BossLevel encoded 1 048 576 0.137 -> 0.125, pixels 1.718 -> 1.710 -- their episodes last hundreds of steps,
    // few waves have a finished env and one launch per step disappears; the single rooms lose -- GoToLocal 65 536 0.035 -> 0.054, PickupLoc
    // 262 144 0.085 -> 0.143 -- 2 % of the envs finish on every step, so most waves carry a reset or two and do them one after the
    // other behind their own step, where k_consume's waves do them all at once.
    return e->cfg.num_rows * e->cfg.num_cols > 1;
}
// One step in three parts, so that bbai_step_render can put the kernel of the batch's second half on another stream:
//   step_prepare  the window gate (fused: the slots this step's waves consume must be there) + what the kernel needs to know about the window
//   step_kernel   k_step over the 64-env blocks [block0, block0 + nblocks) on stream `ks`
//   step_finish   k_consume (unfused) / mission tokens / the window's close + refill -- on the caller's stream, behind EVERY k_step of the step
// what the caller of one step hands over (device pointers); bbai_rollout moves `actions` on from tick to tick
struct StepIO { const uint8_t* actions; uint8_t* image; uint8_t* dirs; float* rewards; double* rewards64; uint8_t* dones; int auto_reset, enum_done;
                int hold;      // the action byte of an env that sits the step out, or -1: none does (step_hold; bbai_bot_rollout: always -1)
};
// The hold byte of a call that is being enqueued (option "step_hold": read here, on the host).
static int step_hold(const bbai_env* e) { return e->step_hold ? BBAI_ACTION_HOLD : -1; }
// What a stepping entry point hands over: its buffers, with the handle's done-action setting and hold byte.
static StepIO step_io(const bbai_env* e, const uint8_t* actions, uint8_t* image, uint8_t* dirs, float* rewards, double* rewards64, uint8_t* dones, int auto_reset) {
    return StepIO{actions, image, dirs, rewards, rewards64, dones, auto_reset, e->done_action_enum, step_hold(e)};
}
struct StepPlan { FuseArgs fa; bool fused; uint32_t* counter; TapArgs tap = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
                  bool dirty = false;      // k_step finds the dirty cells of the registered target for its render (step_render_launch, step_dirty)
};
static int step_prepare(bbai_env* e, int auto_reset, hipStream_t s, StepPlan& p) {
    p.fused = auto_reset && (e->inplace || use_fused_consume(e));
    p.counter = e->counters + 16 * e->step_parity;
    memset(&p.fa, 0, sizeof(p.fa));
    FuseArgs& fa = p.fa;
    if (p.fused) {
        BBAI_TRY(window_begin(e, s));        // the slots this step's waves consume have landed
        const TickPos tp = tick_pos(e);
        fa.next_recs = e->next_rec; fa.next_hots = e->next_hot; fa.next_obs = e->next_obs; fa.depth = e->depth;
        fa.pending = e->pending + (size_t)tp.wb * e->n; fa.first_slot = e->first_slot + (size_t)tp.wb * e->n;
        fa.win_meta = e->win_meta + (size_t)tp.wb * META_U32;
        fa.totals = e->totals;
        e->next_counter_clean = false;      // (a later unfused step clears its ping-pong counter itself)
    } else if (e->inplace) {                // (no auto-reset: the kernel still finds the live records through the ring)
        fa.next_recs = e->next_rec; fa.depth = e->depth;
        if (!e->next_counter_clean) HIP_TRY(hipMemsetAsync(p.counter, 0, 4, s));
        e->next_counter_clean = false;
    } else {
        if (!e->next_counter_clean) HIP_TRY(hipMemsetAsync(p.counter, 0, 4, s));   // (k_consume of the previous step zeroes it)
        e->next_counter_clean = false;
    }
    return BBAI_OK;
}
static int step_kernel(bbai_env* e, const StepPlan& p, const StepIO& io, hipStream_t ks, int64_t block0, int64_t nblocks, int ticks = 1) {
    ProfScope prof_(e, 0, ks);
    if (e->prof_on) e->prof_step_ticks += ticks;
    StepArgs a;
    a.c = e->cfg; a.n = e->n; a.recs = e->rec; a.hots = e->hot; a.stales = e->stale; a.vheads = e->vhead; a.vsets = e->vset; a.actions = io.actions; a.image = io.image; a.dirs = io.dirs;
    a.rewards = io.rewards; a.rewards64 = io.rewards64; a.dones = io.dones; a.auto_reset = io.auto_reset; a.reset_list = e->reset_list; a.reset_slot = e->reset_slot; a.counters = p.counter;
    a.prio = e->step_prio; a.vplane = e->vplane; a.fcache = e->fcache; a.lsm_arr = e->lsm; a.enum_done = io.enum_done; a.hold = io.hold; a.fuse = p.fa; a.block0 = block0; a.cplane = e->cplane;
    a.tap = p.tap; a.ticks = ticks;
    a.dshadow = p.dirty && ticks == 1 ? e->targets.view.shadow : nullptr; a.dmask = e->targets.view.dmask; a.lut = e->lut;
#define STEP_LAUNCH(VV, FF, CC) do { if (ticks > 1) hipLaunchKernelGGL((k_step_ticks<VV, FF, CC>), dim3((unsigned)nblocks), dim3(STEP_BLOCK), 0, ks, a); \
                                     else hipLaunchKernelGGL((k_step<VV, FF, CC>), dim3((unsigned)nblocks), dim3(STEP_BLOCK), 0, ks, a); } while (0)
    if (e->inplace && e->cplane) STEP_LAUNCH(false, 3, true);
    else if (e->inplace) STEP_LAUNCH(false, 3, false);
    else if (p.fused) { if (e->vplane) STEP_LAUNCH(true, 1, false); else STEP_LAUNCH(false, 1, false); }
    else { if (e->vplane) STEP_LAUNCH(true, 0, false); else STEP_LAUNCH(false, 0, false); }
#undef STEP_LAUNCH
    HIP_TRY(hipGetLastError());
    return BBAI_OK;
}
static int step_finish(bbai_env* e, const StepPlan& p, const StepIO& io, hipStream_t s) {
    // the number of finished envs is only known on the device: fixed grids, device-side count
    if (io.auto_reset) return p.fused ? window_end(e, s, 2, io.dones) : consume_and_refill(e, s, io.image, io.dirs, 0);
    return BBAI_OK;
}
static int64_t step_blocks(const bbai_env* e) { return (e->n + STEP_BLOCK - 1) / STEP_BLOCK; }
struct TapRows { uint8_t* image_out; uint8_t* dir_out; double* rew_out; uint8_t* done_out; };
static TapArgs tap_args(const bbai_env* e, const TapRows& r) {       // the rows of bbai_step_tap_set's envs, written by the stepping lanes
    return TapArgs{e->tap_mask, e->tap_rank0, e->tap_perm, r.image_out, r.dir_out, r.rew_out, r.done_out, e->tap_count};
}
// What every stepping entry point asks of the handle first (`what`: "step", or "rollout" in bbai_rollout's messages).
static int step_ready(const bbai_env* e, int auto_reset, const char* what) {
    if (!e->live) { snprintf(g_err, sizeof(g_err), "%s before reset", what); return BBAI_ERR_STATE; }
    if (auto_reset && !e->seeded) {     // live through import_state only: there is no level stream to reset from
        snprintf(g_err, sizeof(g_err), "auto-reset %s before seed", what);
        return BBAI_ERR_STATE;
    }
    return BBAI_OK;
}
static int step_launch(bbai_env* e, const StepIO& io, hipStream_t s, const TapRows* rows = nullptr) {
    StepPlan p;
    BBAI_TRY(step_prepare(e, io.auto_reset, s, p));
    // Inside the stepping waves wherever the step leaves the final outputs behind (fused consume, in-place layout, no auto-reset);
    // an unfused auto-resetting step writes the new episodes' first observations in k_consume: the tap is then a launch behind it.
    const bool in_kernel = rows && (p.fused || e->inplace || !io.auto_reset);
    if (in_kernel) p.tap = tap_args(e, *rows);
    BBAI_TRY(step_kernel(e, p, io, s, 0, step_blocks(e)));
    BBAI_TRY(step_finish(e, p, io, s));
    if (rows && !in_kernel) {
        hipLaunchKernelGGL(k_tap, dim3((unsigned)std::min<int64_t>((e->tap_count * OBS_BYTES + 255) / 256, 2048)), dim3(256), 0, s, e->tap_count, (int64_t)0, e->tap_ids, io.image, io.dirs,
                           io.rewards64, io.dones, (const uint8_t*)nullptr, rows->image_out, rows->dir_out, rows->rew_out, rows->done_out, (uint8_t*)nullptr);
        HIP_TRY(hipGetLastError());
    }
    return BBAI_OK;
}

int bbai_step(bbai_env* e, const uint8_t* actions, uint8_t* image, uint8_t* dirs, float* rewards, double* rewards64,
              uint8_t* dones, int auto_reset, void* stream) {
    if (!e || !actions || !image || !dirs || !rewards || !dones) ARG_FAIL("null handle or buffer");
    BBAI_TRY(step_ready(e, auto_reset, "step"));
    ON_DEVICE(e->device);
    hipStream_t s = (hipStream_t)stream;
    CallScope call(e, s);
    BBAI_TRY(call.rc);
    BBAI_TRY(step_launch(e, step_io(e, actions, image, dirs, rewards, rewards64, dones, auto_reset), s));
    return call.leave();
}

int bbai_step_tap_set(bbai_env* e, const int64_t* ids, int64_t count) {
    if (!e || count < 0 || (count && !ids)) ARG_FAIL("null handle or id list");
    ON_DEVICE(e->device);
    HIP_TRY(hipDeviceSynchronize());
    Owner& o = e->own;      // (the list before goes first: a refused or failing call leaves the handle without one)
    (void)o.drop(&e->tap_mask); (void)o.drop(&e->tap_rank0); (void)o.drop(&e->tap_perm); (void)o.drop(&e->tap_ids); e->tap_count = 0;
    if (count == 0) return BBAI_OK;
    const int64_t nb = (e->n + STEP_BLOCK - 1) / STEP_BLOCK;
    std::vector<unsigned long long> mask((size_t)nb, 0ull);
    std::vector<uint32_t> rank0((size_t)nb, 0u);
    std::vector<int32_t> perm((size_t)count);
    std::vector<std::pair<int64_t, int32_t>> order((size_t)count);
    for (int64_t k = 0; k < count; ++k) {
        if (ids[k] < 0 || ids[k] >= e->n) ARG_FAIL("env id out of range");
        if (mask[(size_t)(ids[k] / STEP_BLOCK)] >> (ids[k] % STEP_BLOCK) & 1ull) ARG_FAIL("an env is listed twice");
        mask[(size_t)(ids[k] / STEP_BLOCK)] |= 1ull << (ids[k] % STEP_BLOCK);
        order[(size_t)k] = {ids[k], (int32_t)k};
    }
    std::sort(order.begin(), order.end());
    for (int64_t k = 0; k < count; ++k) perm[(size_t)k] = order[(size_t)k].second;      // k-th listed env in ascending order -> its log row
    uint32_t run = 0;
    for (int64_t b = 0; b < nb; ++b) { rank0[(size_t)b] = run; run += (uint32_t)__builtin_popcountll(mask[(size_t)b]); }
    BBAI_TRY(o.alloc({{&e->tap_mask, (size_t)nb * 8}, {&e->tap_rank0, (size_t)nb * 4}, {&e->tap_perm, (size_t)count * 4}, {&e->tap_ids, (size_t)count * 8}}));
    HIP_TRY(hipMemcpy(e->tap_mask, mask.data(), (size_t)nb * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->tap_rank0, rank0.data(), (size_t)nb * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->tap_perm, perm.data(), (size_t)count * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->tap_ids, ids, (size_t)count * 8, hipMemcpyHostToDevice));
    e->tap_count = count;
    return BBAI_OK;
}

int bbai_step_tapped(bbai_env* e, const uint8_t* actions, uint8_t* image, uint8_t* dirs, float* rewards, double* rewards64, uint8_t* dones,
                     int auto_reset, uint8_t* image_out, uint8_t* dir_out, double* reward64_out, uint8_t* done_out, void* stream) {
    if (!e || !actions || !image || !dirs || !rewards || !rewards64 || !dones || !image_out || !dir_out || !reward64_out || !done_out) ARG_FAIL("null handle or buffer");
    if (!e->tap_count) { snprintf(g_err, sizeof(g_err), "bbai_step_tapped before bbai_step_tap_set"); return BBAI_ERR_STATE; }
    BBAI_TRY(step_ready(e, auto_reset, "step"));
    ON_DEVICE(e->device);
    hipStream_t s = (hipStream_t)stream;
    CallScope call(e, s);
    BBAI_TRY(call.rc);
    const TapRows rows = {image_out, dir_out, reward64_out, done_out};
    BBAI_TRY(step_launch(e, step_io(e, actions, image, dirs, rewards, rewards64, dones, auto_reset), s, &rows));
    return call.leave();
}

int bbai_set_atlas(bbai_env* e, const uint8_t* tiles, int n_tiles, const uint8_t* lut) {
    if (!e || !tiles || !lut || n_tiles < 1 || n_tiles > MAX_TILES) ARG_FAIL("null pointer or tile count out of range");
    ON_DEVICE(e->device);
    HIP_TRY(hipMemcpy(e->atlas, tiles, (size_t)n_tiles * TILE_BYTES, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->lut, lut, 512, hipMemcpyHostToDevice));
    e->n_tiles = n_tiles;
    target_atlas_replaced(e->targets.view, TILE);      // (a 16 / 32 target: bbai_set_view_atlas)
    return BBAI_OK;
}

int bbai_set_render_target(bbai_env* e, uint8_t* pixels) {
    if (!e) ARG_FAIL("null handle");
    ON_DEVICE(e->device);
    // the first registration: the shadow and the dirty masks, both or neither (un-registering keeps them)
    if (pixels && !e->targets.view.shadow) BBAI_TRY(e->own.alloc({{&e->targets.view.shadow, (size_t)e->n * CELLS}, {&e->targets.view.dmask, (size_t)e->n * sizeof(uint64_t)}}));
    // option "render_target_tile_size": the frames are uint8[n][7 ts][7 ts][3], the shadow holds ids of that size's atlas
    register_target(e->targets.view, (uintptr_t)pixels, e->rt_next_ts, e->n, view_frame_bytes(e->rt_next_ts));
    return BBAI_OK;
}

int bbai_render_invalidate(bbai_env* e) {
    if (!e) ARG_FAIL("null handle");
    invalidate_target(e->targets.view);
    return BBAI_OK;
}

int bbai_render_shadow(bbai_env* e, uint8_t* out, void* stream) {
    if (!e || !out) ARG_FAIL("null handle or buffer");
    if (!e->targets.view.shadow) { snprintf(g_err, sizeof(g_err), "render_shadow before bbai_set_render_target"); return BBAI_ERR_STATE; }
    ON_DEVICE(e->device);
    hipStream_t s = (hipStream_t)stream;
    CallScope call(e, s);
    BBAI_TRY(call.rc);
    HIP_TRY(hipMemcpyAsync(out, e->targets.view.shadow, (size_t)e->n * CELLS, hipMemcpyDeviceToDevice, s));
    return call.leave();
}

}  // extern "C"

// One call that writes frames or observations into a caller's buffer, the only way such a call is made: on the handle's device and inside
// a CallScope, the write is announced to the registered targets (bbai_target.hpp: `write` is a RenderRequest, a GridRenderRequest or a
// WriteRequest), `launch(plan, stream)` enqueues the work and returns a BBAI_* code, and the targets' state moves to what the plan promised
// only when the launches and the call's exit succeeded.
template <class Write, class Launch>
static int frame_call(bbai_env* e, void* stream, const Write& write, Launch launch) {
    ON_DEVICE(e->device);
    hipStream_t s = (hipStream_t)stream;
    CallScope call(e, s);
    BBAI_TRY(call.rc);
    const TargetPlan tp = plan_target(e->targets, write);
    const int rc = [&]() -> int {
        BBAI_TRY(launch(tp, s));
        HIP_TRY(hipGetLastError());
        return call.leave();
    }();
    commit_target(e->targets, tp, rc == BBAI_OK);
    return rc;
}

// A run-time tile size (8, 16 or 32) or view size (3 .. 11, odd) as a compile-time one: f(std::integral_constant).  (The entries have checked both.)
template <int N> using Size = std::integral_constant<int, N>;
template <class F> static void with_tile_size(int ts, F f) { if (ts == 8) f(Size<8>()); else if (ts == 16) f(Size<16>()); else f(Size<32>()); }
template <class F> static void with_view_size(int v, F f) {
    if (v == 3) f(Size<3>()); else if (v == 5) f(Size<5>()); else if (v == 7) f(Size<7>()); else if (v == 9) f(Size<9>()); else f(Size<11>());
}

// Time-paced tickets (option "render_pace", off by default).  k_render_q at the rate of ONE ticket counter (11.4 ns per 8-env ticket
// = 6.6 TB/s) beats every unpaced shape because the counter PACES the chip's stores; a wall-clock gate over two counters can set the
// pace anywhere.  Measured in the step loop on seven boxes (profiles/r04/render_pace_*.jsonl, NOTES section 1): slower than the optimum
// the launch is pace-bound (131 072 tickets x pace), faster it falls off a shallow cliff; at the optimum it beat the one counter by
// 1.5-2.3 % on three boxes (k_render 1.466-1.482 vs 1.50 ms: 0.85 of peak) and LOST 0.5-1.5 % at every pace on two others; the optimum
// moved from 10.8 to 11.4 ns between boxes and between two processes on one box, an idle chip puts it elsewhere than the loop does
// (a first-render tuner), and a perturb-and-observe controller on the launches' own durations paid more for its event pairs and its
// hovering than it gained.  The one counter's 1.50 ms is the same on all of them: it ships; the gate stays as a knob.
static_assert(TARGET_ALIGN_8 == LINE_BYTES && TARGET_UNIT_8 == DELTA_UNIT && TARGET_ALIGN_VIEW == VIEW_PIECE, "bbai_target.hpp restates the delta kernels' store units");
// The full render (what the target's planner, bbai_target.hpp, does not send to the delta render): the queue (queue > 0) or one-shot blocks.
struct RenderPlan {
    uint8_t* shadow;      // a FILL of target envs: their rows of the shadow, where the render also writes every tile id; else NULL
    int queue, pace;      // the queue shape (launch_render_queue; 0: one-shot blocks) and the option "render_pace"
};
static RenderPlan plan_render(const bbai_env* e, uint8_t* shadow) {
    // BBAI_RENDER_QUEUE / option "render_queue": -1 = by batch size (default), 0 = never, m > 0 = queue shape m (launch_render_queue).
    RenderPlan p = {shadow, e->render_queue, e->render_pace};
    if (p.queue < 0) {
        p.queue = e->n >= RENDER_QUEUE_MIN_ENVS ? RENDER_QUEUE_DEFAULT : 0;
        if (p.queue == RENDER_QUEUE_DEFAULT && p.pace > 0) p.queue = RENDER_QUEUE_PACED;        // (a pace needs tickets served faster than it admits them: two counters)
    }
    if (p.pace < 0) p.pace = 0;
    return p;
}

// The grid of a kernel whose persistent blocks share `items` work items (groups, tickets): per_cu blocks on every CU, never more blocks than items.
static int64_t cu_count(const bbai_env* e) { return e->n_cus > 0 ? e->n_cus : 256; }
static unsigned persistent_blocks(const bbai_env* e, int64_t items, int per_cu) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(items, cu_count(e) * per_cu));
}

// One render's range: envs [env_off, env_off + nr) of the batch, `input` and `pixels` at its first env
struct RenderRange { const uint8_t* input; uint8_t* pixels; int64_t nr, env_off; hipStream_t stream; };

// The delta render of target envs whose shadow is valid: behind a step that found the dirty cells the store-only render (k_render_dstore_lw
// for 64-byte pieces, launch_dstore_lw below; k_render_dstore for 128-byte lines and, option "render_delta_sched" 2, for pieces with the
// static split: the previous kernel, kept as the reference), else k_render_delta, of which the following was measured:
// 1 048 576 BossLevel envs, random actions, settings alternated in one process (tools/ab.py; profiles/render_delta/ab.jsonl),
// k_render ms per launch: (1024 threads, 1 block per CU) interleaved 0.813, contiguous ranges 0.795, 2 blocks per CU 0.795;
// (512, 1) 0.795; (512, 3) 0.665 <- default: three independent blocks per CU hide one another's encoding / shadow loads and
// barriers (42 KB of LDS each: three fit).  Full render (k_render_q) 1.507.
template <int T, int SCHED>
static void launch_delta_ts(const bbai_env* e, const RenderRange& r, unsigned blocks, uint8_t* sh) {
    if (e->render_piece_bytes == 128) hipLaunchKernelGGL((k_render_delta<32, T, SCHED, 128>), dim3(blocks), dim3(T), 0, r.stream, r.nr, r.input, r.pixels, sh, e->atlas, e->lut, e->n_tiles);
    else hipLaunchKernelGGL((k_render_delta<32, T, SCHED, 64>), dim3(blocks), dim3(T), 0, r.stream, r.nr, r.input, r.pixels, sh, e->atlas, e->lut, e->n_tiles);
}
template <int T>
static void launch_delta_t(const bbai_env* e, const RenderRange& r, unsigned blocks, uint8_t* sh) {
    if (e->render_delta_sched == 1) launch_delta_ts<T, 1>(e, r, blocks, sh); else launch_delta_ts<T, 0>(e, r, blocks, sh);
}
template <int P>
static void launch_dstore_p(const bbai_env* e, const RenderRange& r, unsigned blocks, uint8_t* sh) {
    hipLaunchKernelGGL((k_render_dstore<32, 512, P>), dim3(blocks), dim3(512), 0, r.stream, r.nr, r.pixels, sh, e->targets.view.dmask + r.env_off, e->atlas, e->n_tiles);
}
// The store-only render of 64-byte pieces (the default): k_render_dstore_lw -- groups from one ticket counter, two per ticket, ONE
// 576-thread block per CU (no more blocks than tickets: every block opens with one).  1 048 576 BossLevel envs, bench.py's actions,
// settings alternated in one process (tools/ab.py; profiles/render_store_queue/), ms per step in five processes: k_render_dstore's static
// split, three blocks per CU, 0.634-0.643; this kernel at three blocks per CU 0.618-0.625, at two 0.621-0.630, at one 0.595-0.610 -- the
// fewer blocks share the one in-order stream of groups, the more compact the window the chip's stores advance through.
static void launch_dstore_lw(const bbai_env* e, const RenderRange& r, int64_t groups, uint8_t* sh) {
    const unsigned blocks = persistent_blocks(e, (groups + DSTORE_LW_K - 1) / DSTORE_LW_K, e->render_delta_bpc > 0 ? e->render_delta_bpc : 1);
    hipLaunchKernelGGL((k_render_dstore_lw<64>), dim3(blocks), dim3(DSTORE_LW_T), 0, r.stream, r.nr, r.pixels, sh, e->targets.view.dmask + r.env_off, e->atlas, e->n_tiles, e->render_tickets);
}
static void launch_render_delta(const bbai_env* e, const RenderRange& r, bool from_step) {
    const int T = e->render_delta_tpb == 1024 && !from_step ? 1024 : 512;
    constexpr int G = 32;
    const int64_t groups = (r.nr + G - 1) / G;
    const unsigned blocks = persistent_blocks(e, groups, e->render_delta_bpc > 0 ? e->render_delta_bpc : (T == 512 ? 3 : 1));
    uint8_t* sh = e->targets.view.shadow + r.env_off * CELLS;
    if (from_step && e->render_piece_bytes != 128 && e->render_delta_sched != 2) launch_dstore_lw(e, r, groups, sh);
    else if (from_step) { if (e->render_piece_bytes == 128) launch_dstore_p<128>(e, r, blocks, sh); else launch_dstore_p<64>(e, r, blocks, sh); }
    else if (T == 512) launch_delta_t<512>(e, r, blocks, sh);
    else launch_delta_t<1024>(e, r, blocks, sh);
}

// From 262 144 envs up: k_render_q -- ONE persistent 1024-thread block per CU, 8-env groups handed out by ONE ticket
// counter.  Everything below was measured inside the step loop, settings alternated in one process (tools/ab.py),
// 1 048 576 BossLevel envs, k_render ms per launch (profiles/r04/render_queue_*.jsonl; four leases = four boxes):
//   one-shot (1024, 8) blocks (rounds 2-3)                         1.64 - 1.72
//   queue, two blocks per CU, one counter (round 3's lead)         1.60 - 1.61
//   queue, ONE block per CU (256 blocks), one counter              1.50            <- shipped: 6.67 TB/s, 0.83 of peak
//   ... 192 / 224 / 320 / 512 blocks                               1.66 / 1.53 / 1.51 / 1.64;   128: 2.14
//   ... two / eight interleaved counters                           1.56 / 1.69 - 1.77
//   ... 2 groups per ticket, 12- / 16-env groups                   1.60 / 1.55 - 1.58 / 1.61
//   ... 512- / 256-thread blocks (8-env groups)                    1.61 - 1.63 / 1.57 (512 blocks)
// One counter serves ~88 M tickets/s (131 072 tickets = 1.49 ms): the shipped shape runs AT the ticket rate, and every
// way of relieving it (more counters, bigger tickets) is slower -- the single counter is what keeps the chip's stores one
// compact, evenly paced window.  By batch size (queue vs the one-shot shape of that size, ms per step): 131 072 envs
// 0.221 vs 0.214, 262 144 0.414 vs 0.418, 393 216 0.614 vs 0.639, 524 288 0.809 vs 0.848 -- below 262 144 the whole
// encoding is still in the memory-side cache and short-lived (512, 2) blocks win.
template <int G, int T, int NC, int K>
static void launch_queue_shape(const bbai_env* e, const RenderRange& r, const RenderPlan& p) {
    static_assert(1024 % T == 0, "1024 / T blocks per CU");
    const int64_t tickets = ((r.nr + G - 1) / G + K - 1) / K;
    const unsigned blocks = e->render_queue_blocks > 0 ? (unsigned)std::max<int64_t>(1, std::min<int64_t>(e->render_queue_blocks, tickets))      // (a count for the whole chip)
                                                        : persistent_blocks(e, tickets, e->render_queue_bpc > 0 ? e->render_queue_bpc : 1024 / T);
    hipLaunchKernelGGL((k_render_q<G, T, NC, K>), dim3(blocks), dim3(T), 0, r.stream, r.nr, r.input, r.pixels, e->atlas, e->lut, e->n_tiles, e->render_tickets, p.pace, p.shadow);
}
static void launch_render_queue(const bbai_env* e, const RenderRange& r, const RenderPlan& p) {
    switch (p.queue) {     // (shapes other than 1 stay for measurements: tests/test_gpu_parity.py checks every one byte for byte)
    default:
    case 1: launch_queue_shape<8, 1024, 1, 1>(e, r, p); break;       // shipped
    case 2: launch_queue_shape<8, 1024, 8, 1>(e, r, p); break;       // eight / two interleaved counters
    case 3: launch_queue_shape<8, 1024, 2, 1>(e, r, p); break;
    case 4: launch_queue_shape<8, 1024, 1, 2>(e, r, p); break;       // two groups per ticket
    case 5: launch_queue_shape<12, 1024, 1, 1>(e, r, p); break;      // bigger groups
    case 6: launch_queue_shape<16, 1024, 1, 1>(e, r, p); break;
    case 7: launch_queue_shape<8, 512, 1, 1>(e, r, p); break;        // smaller blocks
    case 8: launch_queue_shape<8, 256, 1, 1>(e, r, p); break;
    case 9: launch_queue_shape<2, 512, 8, 1>(e, r, p); break;        // small groups need more counters (524 288 tickets)
    case 10: launch_queue_shape<9, 1024, 1, 1>(e, r, p); break;      // just above the shipped group: a little more work per ticket
    case 11: launch_queue_shape<10, 1024, 1, 1>(e, r, p); break;
    }
}

// ONE G-env group per one-shot block of T threads, (512, 2) (round 2: profiles/r02/render_shape_*.jsonl; (1024, 8) from
// 786 432 envs when the queue is switched off).  BBAI_RENDER_GROUP / BBAI_RENDER_TPB override (experiments).
template <int G>
static void launch_oneshot_g(const bbai_env* e, const RenderRange& r, int T, uint8_t* shadow) {
    const dim3 grid((unsigned)((r.nr + G - 1) / G));
    if (T == 1024) hipLaunchKernelGGL((k_render<G, 1024>), grid, dim3(1024), 0, r.stream, r.nr, r.input, r.pixels, e->atlas, e->lut, e->n_tiles, shadow);
    else if (T == 512) hipLaunchKernelGGL((k_render<G, 512>), grid, dim3(512), 0, r.stream, r.nr, r.input, r.pixels, e->atlas, e->lut, e->n_tiles, shadow);
    else hipLaunchKernelGGL((k_render<G, 256>), grid, dim3(256), 0, r.stream, r.nr, r.input, r.pixels, e->atlas, e->lut, e->n_tiles, shadow);
}
static void launch_render_oneshot(const bbai_env* e, const RenderRange& r, uint8_t* shadow) {
    const bool big = e->n >= 786432;
    int G = e->render_group, T = e->render_tpb;
    if (G != 2 && G != 4 && G != 8) G = big ? 8 : 2;
    if (T != 256 && T != 512 && T != 1024) T = big ? 1024 : 512;
    if (G == 2) launch_oneshot_g<2>(e, r, T, shadow); else if (G == 4) launch_oneshot_g<4>(e, r, T, shadow); else launch_oneshot_g<8>(e, r, T, shadow);
}

static int render_launch(bbai_env* e, const uint8_t* input, uint8_t* pixels, void* stream, int64_t n_render = -1 /* envs input / pixels hold (default: the batch); the shape follows the BATCH size */,
                         int64_t env_off = 0 /* first env of the range (bbai_step_render's split halves) */,
                         bool from_step = false /* the step in front found the dirty cells (step_dirty): store them (k_render_dstore) */) {
    const RenderRange r = {input, pixels, n_render < 0 ? e->n : n_render, env_off, (hipStream_t)stream};
    // envs of the target go to the delta render or, while the shadow is not valid, to the full render, which then also writes every tile id
    return frame_call(e, stream, RenderRequest{TILE, (uintptr_t)pixels, r.nr * (int64_t)PIX_BYTES, env_off, r.nr, false, e->render_delta != 0}, [&](const TargetPlan& tp, hipStream_t) {
        ProfScope prof_(e, 2, r.stream);
        const RenderPlan p = plan_render(e, tp.kind == TargetPlan::FILL ? e->targets.view.shadow + tp.shadow_off : nullptr);
        if (tp.kind == TargetPlan::DELTA) launch_render_delta(e, r, from_step);
        else if (p.queue > 0) launch_render_queue(e, r, p);
        else launch_render_oneshot(e, r, p.shadow);
        return BBAI_OK;
    });
}

extern "C" {

int bbai_render(bbai_env* e, const uint8_t* image, uint8_t* pixels, void* stream) {
    if (!e || !image || !pixels) ARG_FAIL("null handle or buffer");
    if (e->n_tiles <= 0) { snprintf(g_err, sizeof(g_err), "render before set_atlas"); return BBAI_ERR_STATE; }
    return render_launch(e, image, pixels, stream);
}

// ---- the full-grid picture (k_render_grid) ----
static int grid_ts_index(int ts) { return ts == 8 ? 0 : ts == 16 ? 1 : ts == 32 ? 2 : -1; }

// One installer for the full-grid atlases and the view's (`who`: they differ in constants alone), into slot k of the handle's atlas / lookup table / tile count arrays.
// The first installation at a tile size allocates both buffers or neither; a later one reuses them.  (The callers have checked the handle, the pointers and the tile size.)
static int atlas_install(bbai_env* e, const char* who, uint8_t** atlas, uint8_t** lut_dev, int* installed, int k, int tile_size, int max_tiles, int lut_bytes,
                         const uint8_t* tiles, int n_tiles, const uint8_t* lut) {
    if (n_tiles < 1 || n_tiles > max_tiles) { snprintf(g_err, sizeof(g_err), "%s: %s", who, "tile count out of range"); return BBAI_ERR_ARG; }
    for (int i = 0; i < lut_bytes; ++i)
        if (lut[i] >= n_tiles) { snprintf(g_err, sizeof(g_err), "%s: %s", who, "a lut entry names a tile the atlas does not hold"); return BBAI_ERR_ARG; }
    ON_DEVICE(e->device);
    const size_t tb = (size_t)tile_size * tile_size * 3;
    HIP_TRY(hipDeviceSynchronize());                 // (a render still in flight may read the atlas being replaced)
    if (!atlas[k]) BBAI_TRY(e->own.alloc({{&atlas[k], (size_t)(max_tiles + 1) * tb}, {&lut_dev[k], (size_t)lut_bytes}}));
    HIP_TRY(hipMemcpy(atlas[k], tiles, n_tiles * tb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(atlas[k] + n_tiles * tb, 0, tb));        // the zero tile: frames of ids (grid) / row ids (view) outside the batch
    HIP_TRY(hipMemcpy(lut_dev[k], lut, (size_t)lut_bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipDeviceSynchronize());
    installed[k] = n_tiles;
    return BBAI_OK;
}

int bbai_set_grid_atlas(bbai_env* e, int tile_size, const uint8_t* tiles, int n_tiles, const uint8_t* lut) {
    const int k = grid_ts_index(tile_size);
    if (!e || !tiles || !lut) ARG_FAIL("null handle or pointer");
    if (k < 0) ARG_FAIL("tile size must be 8, 16 or 32");
    target_atlas_replaced(e->targets.grid, tile_size);
    return atlas_install(e, __func__, e->grid_atlas, e->grid_lut, e->grid_tiles, k, tile_size, GRID_MAX_TILES, GRID_LUT_BYTES, tiles, n_tiles, lut);
}

}  // extern "C"

// ---- observations of listed envs from the live state: render_grid, observe_full, observe_view (bbai_kernels.hpp: EnvList) ----
static EnvList env_list(const bbai_env* e, const int64_t* ids, int64_t count, uint8_t* out) {
    return EnvList{e->cfg, e->n, e->rec, e->inplace ? e->next_rec : nullptr, e->depth, e->hot, ids, count, out};
}
// The frames' buffer of a call that draws `count` frames: there, and 16-byte aligned (the kernels store 16-byte chunks).
static int frames_ready(const char* func, int64_t count, const uint8_t* out) {
    if (count > 0 && (!out || ((uintptr_t)out & 15))) { snprintf(g_err, sizeof(g_err), "%s: output buffer missing or not 16-byte aligned", func); return BBAI_ERR_ARG; }
    return BBAI_OK;
}
// What those three entry points (`func`: "bbai_<who>") ask first, in the order their callers have always seen: the count, the frames'
// buffer, then the state -- render_grid's atlas (no_atlas_ts: the tile size that has none, else 0) in front of "<who> before reset".
static int listed_ready(const bbai_env* e, const char* func, const int64_t* ids, int64_t count, const uint8_t* out, int no_atlas_ts = 0) {
    const char* who = func + 5;
    if (count < 0 || (!ids && count > e->n)) { snprintf(g_err, sizeof(g_err), "%s: env count out of range", func); return BBAI_ERR_ARG; }
    BBAI_TRY(frames_ready(func, count, out));
    if (no_atlas_ts) { snprintf(g_err, sizeof(g_err), "%s: no atlas for tile size %d (bbai_set_grid_atlas)", who, no_atlas_ts); return BBAI_ERR_STATE; }
    if (!e->live) { snprintf(g_err, sizeof(g_err), "%s before reset", who); return BBAI_ERR_STATE; }
    return BBAI_OK;
}

// Launch shape by frame size F: small frames (F <= 64 KB: GoToLocal at tile size 8 is 12 KB) -- several envs per work item, about 128 KB
// of frames each; large ones (BossLevel at 32: 1.49 MB) -- an env in slices of about 256 KB.  Persistent blocks: 2 per CU at tile sizes 8
// and 32 (35 KB / 10 KB of LDS), 1 at 16 (the 102 KB atlas); option "grid_render_bpc" overrides.
template <int TS>
static void render_grid_launch(bbai_env* e, int highlight, const int64_t* ids, int64_t count, uint8_t* out, hipStream_t s) {
    const int k = grid_ts_index(TS);
    const LevelCfg& c = e->cfg;
    const int64_t F = (int64_t)c.H * TS * c.W * TS * 3;
    GridArgs a;
    a.list = env_list(e, ids, count, out);
    a.atlas = e->grid_atlas[k]; a.lut = e->grid_lut[k]; a.n_tiles = e->grid_tiles[k];
    a.highlight = highlight ? 1 : 0;
    a.envs_per_item = 1; a.slices = 1;
    if (F <= 65536) a.envs_per_item = (int)std::max<int64_t>(1, std::min<int64_t>({131072 / F, GRID_MAX_ENVS, GRID_ID_BYTES / (c.W * c.H)}));
    else a.slices = (int)std::max<int64_t>(1, F / 262144);
    a.items = a.slices > 1 ? count * a.slices : (count + a.envs_per_item - 1) / a.envs_per_item;
    a.frame16 = (uint32_t)(F / 16);
    a.frame_magic = (1ull << 32) / a.frame16 + 1;
    a.ppr = (uint32_t)(c.W * TS * 3 / GridTile<TS>::P);
    a.ppr_magic = (1ull << 32) / a.ppr + 1;
    const unsigned blocks = persistent_blocks(e, a.items, e->grid_bpc > 0 ? e->grid_bpc : (TS == 16 ? 1 : 2));
    hipLaunchKernelGGL((k_render_grid<TS>), dim3(blocks), dim3(GRID_BLOCK), 0, s, a);
}

extern "C" {

int bbai_render_grid(bbai_env* e, int tile_size, int highlight, const int64_t* ids, int64_t count, uint8_t* out, void* stream) {
    const int k = grid_ts_index(tile_size);
    if (!e) ARG_FAIL("null handle");
    if (k < 0) ARG_FAIL("tile size must be 8, 16 or 32");
    BBAI_TRY(listed_ready(e, __func__, ids, count, out, e->grid_tiles[k] ? 0 : tile_size));
    if (count == 0) return BBAI_OK;
    return frame_call(e, stream, WriteRequest{(uintptr_t)out, count * grid_frame_bytes(e->cfg.W * e->cfg.H, tile_size)}, [&](const TargetPlan&, hipStream_t s) {
        with_tile_size(tile_size, [&](auto ts) { render_grid_launch<ts()>(e, highlight, ids, count, out, s); });
        return BBAI_OK;
    });
}

}  // extern "C"

// ---- the 7x7 view as pixels at tile sizes 16 / 32 (k_view_pixels) ----
static int view_ts_index(int ts) { return ts == 16 ? 0 : ts == 32 ? 1 : -1; }

extern "C" {

int bbai_set_view_atlas(bbai_env* e, int tile_size, const uint8_t* tiles, int n_tiles, const uint8_t* lut) {
    const int k = view_ts_index(tile_size);
    if (!e || !tiles || !lut) ARG_FAIL("null handle or pointer");
    if (k < 0) ARG_FAIL("tile size must be 16 or 32 (8: bbai_set_atlas)");
    target_atlas_replaced(e->targets.view, tile_size);
    return atlas_install(e, __func__, e->view_atlas, e->view_lut, e->view_tiles, k, tile_size, VIEWPX_MAX_TILES, VIEWPX_LUT_BYTES, tiles, n_tiles, lut);
}

}  // extern "C"

// Launch shape: work items of about 150 KB of frames -- 4 envs at tile size 16, one env at 32, or half an env while there are fewer
// frames than blocks (a few frames still reach every CU); persistent blocks, two per CU.
template <int TS>
static void render_view_launch(bbai_env* e, const uint8_t* image, int64_t rows, const int64_t* ids, int64_t count, uint8_t* out, hipStream_t s) {
    const int k = view_ts_index(TS);
    const int64_t want = cu_count(e) * 2;
    ViewPxArgs a;
    a.image = image; a.rows = rows; a.ids = ids; a.count = count; a.out = out;
    a.atlas = e->view_atlas[k]; a.lut = e->view_lut[k]; a.n_tiles = e->view_tiles[k];
    a.envs_per_item = TS == 16 ? VIEWPX_MAX_ENVS : 1;
    a.slices = TS == 32 && count < want ? 2 : 1;
    a.items = a.slices > 1 ? count * a.slices : (count + a.envs_per_item - 1) / a.envs_per_item;
    const unsigned blocks = persistent_blocks(e, a.items, 2);
    hipLaunchKernelGGL((k_view_pixels<TS>), dim3(blocks), dim3(VIEWPX_BLOCK), 0, s, a);
}

// A whole batch into the registered target of tile size TS (the planner has said that this is such a call).  DELTA: k_view_delta, persistent
// blocks, two per CU, over static groups of 16 / 8 envs.  FILL: the frames whole (k_view_pixels, unchanged) and every tile id behind them
// (k_view_ids).
template <int TS>
static void view_delta_launch(bbai_env* e, bool fill, const uint8_t* image, uint8_t* out, hipStream_t s) {
    const int k = view_ts_index(TS);
    if (fill) {
        render_view_launch<TS>(e, image, e->n, nullptr, e->n, out, s);
        hipLaunchKernelGGL(k_view_ids, dim3(persistent_blocks(e, (e->n * CELLS + 255) / 256, 8)), dim3(256), 0, s, image, e->n, e->view_lut[k], e->targets.view.shadow);
        return;
    }
    ViewDeltaArgs a;
    a.image = image; a.n = e->n; a.out = out; a.shadow = e->targets.view.shadow;
    a.atlas = e->view_atlas[k]; a.lut = e->view_lut[k]; a.n_tiles = e->view_tiles[k];
    const int64_t groups = (e->n + ViewDelta<TS>::G - 1) / ViewDelta<TS>::G;
    hipLaunchKernelGGL((k_view_delta<TS>), dim3(persistent_blocks(e, groups, 2)), dim3(VIEWDELTA_BLOCK), 0, s, a);
}

extern "C" {

int bbai_render_view(bbai_env* e, int tile_size, const uint8_t* image, int64_t rows, const int64_t* ids, int64_t count, uint8_t* out, void* stream) {
    const int k = view_ts_index(tile_size);
    if (!e) ARG_FAIL("null handle");
    if (k < 0) ARG_FAIL("tile size must be 16 or 32 (8: bbai_render)");
    if (rows < 0 || count < 0 || (!ids && count > rows)) ARG_FAIL("row count out of range");
    if (count > 0 && rows > 0 && !image) ARG_FAIL("encoded buffer missing");
    BBAI_TRY(frames_ready(__func__, count, out));
    if (!e->view_tiles[k]) { snprintf(g_err, sizeof(g_err), "render_view: no atlas for tile size %d (bbai_set_view_atlas)", tile_size); return BBAI_ERR_STATE; }
    if (count == 0) return BBAI_OK;
    // the whole batch into the target registered at this tile size is a delta render (or, while the shadow is not valid, the whole frames
    // with every tile id behind them); anything else -- ids given, a partial count, another tile size, a misaligned target,
    // "render_delta" 0 -- draws whole frames, and invalidates where it writes into a registered buffer
    const RenderRequest q = {tile_size, (uintptr_t)out, count * view_frame_bytes(tile_size), 0, count, ids || count != rows || rows != e->n, e->render_delta != 0};
    return frame_call(e, stream, q, [&](const TargetPlan& tp, hipStream_t s) {
        if (tp.kind == TargetPlan::ELSEWHERE) { if (k == 0) render_view_launch<16>(e, image, rows, ids, count, out, s); else render_view_launch<32>(e, image, rows, ids, count, out, s); }
        else if (k == 0) view_delta_launch<16>(e, tp.kind == TargetPlan::FILL, image, out, s);
        else view_delta_launch<32>(e, tp.kind == TargetPlan::FILL, image, out, s);
        return BBAI_OK;
    });
}

}  // extern "C"

// ---- the V x V view as pixels, view sizes 3 .. 11 at tile sizes 8 / 16 / 32 (include/bbai_view_pixels.h: k_view_pixels_n) ----
// Launch shape: viewpxn_items' work items (bbai_viewpxn.hpp), persistent blocks, two per CU.
template <int V, int TS>
static void view_pixels_launch_vt(bbai_env* e, const uint8_t* image, int64_t rows, const int64_t* ids, int64_t count, uint8_t* out, hipStream_t s) {
    const int k = grid_ts_index(TS);
    const ViewPxItems it = viewpxn_items(V, TS, count, cu_count(e) * 2);
    ViewPxArgs a;
    a.image = image; a.rows = rows; a.ids = ids; a.count = count; a.out = out;
    a.atlas = e->vpx_atlas[k]; a.lut = e->vpx_lut[k]; a.n_tiles = e->vpx_tiles[k];
    a.envs_per_item = it.envs_per_item; a.slices = it.slices; a.items = it.items;
    hipLaunchKernelGGL((k_view_pixels_n<V, TS>), dim3(persistent_blocks(e, a.items, 2)), dim3(VIEWPXN_BLOCK), 0, s, a);
}

extern "C" {

int bbai_set_view_pixels_atlas(bbai_env* e, int tile_size, const uint8_t* tiles, int n_tiles, const uint8_t* lut) {
    const int k = grid_ts_index(tile_size);
    if (!e || !tiles || !lut) ARG_FAIL("null handle or pointer");
    if (k < 0) ARG_FAIL("tile size must be 8, 16 or 32");
    // (this entry's own atlases: no registered target's frame was drawn with them, so no history to invalidate)
    return atlas_install(e, __func__, e->vpx_atlas, e->vpx_lut, e->vpx_tiles, k, tile_size, VIEWPX_MAX_TILES, VIEWPX_LUT_BYTES, tiles, n_tiles, lut);
}

int bbai_render_view_pixels(bbai_env* e, int view_size, int tile_size, const uint8_t* image, int64_t rows, const int64_t* ids, int64_t count,
                            uint8_t* out, void* stream) {
    const int k = grid_ts_index(tile_size);
    if (!e) ARG_FAIL("null handle");
    if (!viewpxn_view_ok(view_size)) ARG_FAIL("view size must be 3, 5, 7, 9 or 11");
    if (k < 0) ARG_FAIL("tile size must be 8, 16 or 32");
    if (rows < 0 || count < 0 || (!ids && count > rows)) ARG_FAIL("row count out of range");
    if (count > 0 && rows > 0 && !image) ARG_FAIL("encoded buffer missing");
    BBAI_TRY(frames_ready(__func__, count, out));
    if (!e->vpx_tiles[k]) { snprintf(g_err, sizeof(g_err), "render_view_pixels: no atlas for tile size %d (bbai_set_view_pixels_atlas)", tile_size); return BBAI_ERR_STATE; }
    if (count == 0) return BBAI_OK;
    // never a render of target envs into their own rows: whole frames, and where they land in a registered buffer its history is gone
    return frame_call(e, stream, WriteRequest{(uintptr_t)out, count * (int64_t)(3 * view_size * view_size * tile_size * tile_size)}, [&](const TargetPlan&, hipStream_t s) {
        with_view_size(view_size, [&](auto v) { with_tile_size(tile_size, [&](auto ts) { view_pixels_launch_vt<v(), ts()>(e, image, rows, ids, count, out, s); }); });
        return BBAI_OK;
    });
}

}  // extern "C"

// Launch shape: items of as many envs as fit FULL_LDS and FULL_APP (at most FULL_MAX_ENVS), a multiple of 16 / gcd(F, 16) so that every
// item's range of `out` starts on a 16-byte boundary (the largest grids with an odd F, 25 x 25 at ES 36, would need 16 x 1875 B: refused,
// no level has one -- BossLevel: 16 envs, 23 232 B of frames, 11 264 B of rows); persistent blocks, FULL_BPC per CU.
static int full_launch(bbai_env* e, const int64_t* ids, int64_t count, uint8_t* out, hipStream_t s) {
    const LevelCfg& c = e->cfg;
    const int F = 3 * c.W * c.H;
    int g = 16;
    while (F % g) g >>= 1;                                // gcd(F, 16)
    const int align = 16 / g;
    const int epi = std::min({FULL_MAX_ENVS, FULL_LDS / F, FULL_APP / (c.H * c.ES)}) / align * align;
    if (epi < 1) { snprintf(g_err, sizeof(g_err), "observe_full: grid %d x %d too large", c.W, c.H); return BBAI_ERR_ARG; }
    FullArgs a;
    a.list = env_list(e, ids, count, out);
    a.envs_per_item = epi;
    a.items = (count + epi - 1) / epi;
    a.hw_magic = (1ull << 32) / (uint32_t)(c.W * c.H) + 1;
    a.w_magic = (1ull << 32) / (uint32_t)c.W + 1;
    a.rd_magic = (1ull << 32) / (uint32_t)(c.H * c.ES / 4) + 1;
    hipLaunchKernelGGL(k_full_obs, dim3(persistent_blocks(e, a.items, FULL_BPC)), dim3(FULL_BLOCK), 0, s, a);
    return BBAI_OK;
}

// The view-size entries (include/bbai_view_size.h).  Launch shape of k_view_obs<V>: items of ViewN<V>::EPI envs, persistent blocks, VIEWN_BPC per CU.
template <int V>
static void viewn_launch_v(bbai_env* e, const int64_t* ids, int64_t count, uint8_t* out, hipStream_t s) {
    ViewNArgs a;
    a.list = env_list(e, ids, count, out);
    a.items = (count + ViewN<V>::EPI - 1) / ViewN<V>::EPI;
    hipLaunchKernelGGL((k_view_obs<V>), dim3(persistent_blocks(e, a.items, VIEWN_BPC)), dim3(VIEWN_BLOCK), 0, s, a);
}

// One observation launch of either kind (view_size 0: the fully observable encoding; the entry has checked the size) of `count` frames
// into the WriteRequest's bytes, and the two calls built on it: the listed envs' frames (the entry point has asked listed_ready), and a
// step of the whole batch with every env's frame behind it, as one call.
static WriteRequest observe_write(const bbai_env* e, int view_size, int64_t count, const uint8_t* out) {
    return WriteRequest{(uintptr_t)out, count * (int64_t)(view_size ? 3 * view_size * view_size : 3 * e->cfg.W * e->cfg.H)};
}
static int observe_launch(bbai_env* e, int view_size, const int64_t* ids, int64_t count, uint8_t* out, hipStream_t s) {
    if (!view_size) return full_launch(e, ids, count, out, s);
    with_view_size(view_size, [&](auto v) { viewn_launch_v<v()>(e, ids, count, out, s); });
    return BBAI_OK;
}
static int observe_listed(bbai_env* e, int view_size, const int64_t* ids, int64_t count, uint8_t* out, void* stream) {
    if (count == 0) return BBAI_OK;
    return frame_call(e, stream, observe_write(e, view_size, count, out), [&](const TargetPlan&, hipStream_t s) { return observe_launch(e, view_size, ids, count, out, s); });
}
static int step_observe(bbai_env* e, const StepIO& io, int view_size, uint8_t* frames, void* stream) {
    BBAI_TRY(step_ready(e, io.auto_reset, "step"));
    return frame_call(e, stream, observe_write(e, view_size, e->n, frames), [&](const TargetPlan&, hipStream_t s) -> int {
        BBAI_TRY(step_launch(e, io, s));
        return observe_launch(e, view_size, nullptr, e->n, frames, s);
    });
}

extern "C" {

int bbai_observe_full(bbai_env* e, const int64_t* ids, int64_t count, uint8_t* out, void* stream) {
    if (!e) ARG_FAIL("null handle");
    BBAI_TRY(listed_ready(e, __func__, ids, count, out));
    return observe_listed(e, 0, ids, count, out, stream);
}

int bbai_step_full(bbai_env* e, const uint8_t* actions, uint8_t* image, uint8_t* dirs, float* rewards, double* rewards64,
                   uint8_t* dones, int auto_reset, uint8_t* full, void* stream) {
    if (!e || !actions || !image || !dirs || !rewards || !dones || !full) ARG_FAIL("null handle or buffer");
    if ((uintptr_t)full & 15) ARG_FAIL("full observation buffer not 16-byte aligned");
    return step_observe(e, step_io(e, actions, image, dirs, rewards, rewards64, dones, auto_reset), 0, full, stream);
}

int bbai_observe_view(bbai_env* e, int view_size, const int64_t* ids, int64_t count, uint8_t* out, void* stream) {
    if (!e) ARG_FAIL("null handle");
    if (!view_size_ok(view_size)) ARG_FAIL("view size must be 3, 5, 7, 9 or 11");
    BBAI_TRY(listed_ready(e, __func__, ids, count, out));
    return observe_listed(e, view_size, ids, count, out, stream);
}

int bbai_step_view(bbai_env* e, const uint8_t* actions, uint8_t* image, uint8_t* dirs, float* rewards, double* rewards64,
                   uint8_t* dones, int auto_reset, int view_size, uint8_t* view, void* stream) {
    if (!e || !actions || !image || !dirs || !rewards || !dones || !view) ARG_FAIL("null handle or buffer");
    if (!view_size_ok(view_size)) ARG_FAIL("view size must be 3, 5, 7, 9 or 11");
    if ((uintptr_t)view & 15) ARG_FAIL("view observation buffer not 16-byte aligned");
    return step_observe(e, step_io(e, actions, image, dirs, rewards, rewards64, dones, auto_reset), view_size, view, stream);
}

}  // extern "C"

// ---- the registered full-grid target (include/bbai_grid_target.h; bbai_target.hpp: record and planner; bbai_gridtarget.hpp: the pieces; bbai_griddelta.hpp: k_grid_delta) ----
// The whole batch into the registered buffer.  DELTA: k_grid_delta<TS>, persistent blocks, GRIDDELTA_BPC per CU, over static groups of
// griddelta_shape's envs (bbai_gridtarget.hpp; option "grid_delta_group").  FILL: the frames whole (k_render_grid<TS>, unchanged) and every
// tile id behind them (k_grid_ids).
template <int TS>
static void grid_target_launch(bbai_env* e, bool fill, hipStream_t s) {
    const int k = grid_ts_index(TS);
    const LevelCfg& c = e->cfg;
    uint8_t* const out = (uint8_t*)e->targets.grid.pixels;
    if (fill) {
        render_grid_launch<TS>(e, 0, nullptr, e->n, out, s);
        hipLaunchKernelGGL(k_grid_ids, dim3(persistent_blocks(e, (e->n * c.W * c.H + 255) / 256, 8)), dim3(256), 0, s, env_list(e, nullptr, e->n, out), e->grid_lut[k], e->targets.grid.shadow);
        return;
    }
    const int64_t want = cu_count(e) * GRIDDELTA_BPC;
    GridDeltaArgs a;
    a.g.list = env_list(e, nullptr, e->n, out);
    a.g.atlas = e->grid_atlas[k]; a.g.lut = e->grid_lut[k]; a.g.n_tiles = e->grid_tiles[k];
    a.g.highlight = 0; a.g.envs_per_item = 1; a.g.slices = 1; a.g.items = 0;
    a.g.frame16 = (uint32_t)((int64_t)c.H * TS * c.W * TS * 3 / 16);
    a.g.frame_magic = (1ull << 32) / a.g.frame16 + 1;
    a.g.ppr = (uint32_t)(c.W * TS * 3 / GridTile<TS>::P);
    a.g.ppr_magic = (1ull << 32) / a.g.ppr + 1;
    a.shadow = e->targets.grid.shadow;
    a.geom = grid_geom(c.W, c.H, TS);
    const GridDeltaShape shape = griddelta_shape(e->n, want, c.W, c.H, c.ES, e->grid_delta_group);
    a.envs_per_group = shape.envs_per_group;
    a.groups = shape.groups;
    a.hw_magic = (1ull << 32) / (uint32_t)(c.W * c.H) + 1;
    a.w_magic = (1ull << 32) / (uint32_t)c.W + 1;
    a.rd_magic = (1ull << 32) / (uint32_t)(c.H * c.ES / 4) + 1;
    hipLaunchKernelGGL((k_grid_delta<TS>), dim3(persistent_blocks(e, a.groups, GRIDDELTA_BPC)), dim3(GRIDDELTA_BLOCK), 0, s, a);
}
static_assert(GRID_TARGET_ALIGN == GRID_PIECE, "the registered buffer starts on a piece");

// What a render into the target asks of the handle first (`func`: "bbai_<who>").
static int grid_target_ready(const bbai_env* e, const char* func) {
    const char* who = func + 5;
    if (!e->targets.grid.pixels) { snprintf(g_err, sizeof(g_err), "%s: no grid target (bbai_set_grid_target)", who); return BBAI_ERR_STATE; }
    if (!e->grid_tiles[grid_ts_index(e->targets.grid.ts)]) { snprintf(g_err, sizeof(g_err), "%s: no atlas for tile size %d (bbai_set_grid_atlas)", who, e->targets.grid.ts); return BBAI_ERR_STATE; }
    if (!e->live) { snprintf(g_err, sizeof(g_err), "%s before reset", who); return BBAI_ERR_STATE; }
    return BBAI_OK;
}
// The render into the target -- behind the step's launches where `io` names a step -- as one call.  Where the registered buffer lies over
// the 7x7 view's target that one's history is gone (bbai_target.hpp).
static int grid_target_call(bbai_env* e, const StepIO* io, void* stream) {
    return frame_call(e, stream, GridRenderRequest{e->grid_render_delta != 0}, [&](const TargetPlan& tp, hipStream_t s) -> int {
        if (io) BBAI_TRY(step_launch(e, *io, s));
        with_tile_size(e->targets.grid.ts, [&](auto ts) { grid_target_launch<ts()>(e, tp.kind == TargetPlan::FILL, s); });
        return BBAI_OK;
    });
}

extern "C" {

int bbai_set_grid_target(bbai_env* e, uint8_t* frames, int tile_size) {
    if (!e) ARG_FAIL("null handle");
    if (grid_ts_index(tile_size) < 0) ARG_FAIL("tile size must be 8, 16 or 32");
    if ((uintptr_t)frames % GRID_TARGET_ALIGN) ARG_FAIL("grid target not 64-byte aligned");
    if (frames && !grid_geom_ok(e->cfg.W, e->cfg.H, tile_size)) ARG_FAIL("grid too narrow for 64-byte pieces");
    ON_DEVICE(e->device);
    // the first registration: the shadow (un-registering keeps it)
    if (frames && !e->targets.grid.shadow) BBAI_TRY(e->own.alloc({{&e->targets.grid.shadow, (size_t)e->n * e->cfg.W * e->cfg.H}}));
    register_target(e->targets.grid, (uintptr_t)frames, tile_size, e->n, grid_frame_bytes((int64_t)e->cfg.W * e->cfg.H, tile_size));
    return BBAI_OK;
}

int bbai_grid_target_invalidate(bbai_env* e) {
    if (!e) ARG_FAIL("null handle");
    invalidate_target(e->targets.grid);
    return BBAI_OK;
}

int bbai_grid_target_shadow(bbai_env* e, uint8_t* out, void* stream) {
    if (!e || !out) ARG_FAIL("null handle or buffer");
    if (!e->targets.grid.shadow) { snprintf(g_err, sizeof(g_err), "grid_target_shadow before bbai_set_grid_target"); return BBAI_ERR_STATE; }
    ON_DEVICE(e->device);
    hipStream_t s = (hipStream_t)stream;
    CallScope call(e, s);
    BBAI_TRY(call.rc);
    HIP_TRY(hipMemcpyAsync(out, e->targets.grid.shadow, (size_t)e->n * e->cfg.W * e->cfg.H, hipMemcpyDeviceToDevice, s));
    return call.leave();
}

int bbai_render_grid_target(bbai_env* e, void* stream) {
    if (!e) ARG_FAIL("null handle");
    BBAI_TRY(grid_target_ready(e, __func__));
    return grid_target_call(e, nullptr, stream);
}

int bbai_step_grid_target(bbai_env* e, const uint8_t* actions, uint8_t* image, uint8_t* dirs, float* rewards, double* rewards64,
                          uint8_t* dones, int auto_reset, void* stream) {
    if (!e || !actions || !image || !dirs || !rewards || !dones) ARG_FAIL("null handle or buffer");
    BBAI_TRY(grid_target_ready(e, __func__));
    BBAI_TRY(step_ready(e, auto_reset, "step"));
    const StepIO io = step_io(e, actions, image, dirs, rewards, rewards64, dones, auto_reset);
    return grid_target_call(e, &io, stream);
}

}  // extern "C"

// step + render of a pixel batch as ONE call.  The render is a pure store stream at the chip's fill rate (k_render_q: 1.50 ms per
// 1 048 576 envs) and k_step (0.10 ms) runs in FRONT of it with the store pipes idle -- 6 % of the headline step.  Split (option
// "step_render_split" = 1): the batch is stepped in two halves; the second half's k_step goes to a stream of its own and runs UNDER the
// first half's render (the render's blocks hold 56 VGPRs and 20 KB of LDS per CU: room for k_step's waves next to them):
//     caller's stream:  gate . k_step(A) . k_render(A) ........ [wait B] . tokens / window close . k_render(B)
//     split stream:             k_step(B) ........
// Same kernels, same bytes (tests/test_gpu_parity.py::test_step_render_split_*).  MEASURED SLOWER at every size, settings alternated in
// one process (profiles/r05/step_render_split_ab.jsonl, ms per step unsplit / split): 1 048 576 envs 1.599 / 1.609, 524 288 0.806 / 0.808,
// 262 144 0.413 / 0.423, 131 072 0.210 / 0.222 -- the two half renders together cost more than the one (0.7565 x 2 vs 1.5007 ms: the
// store stream's pacing restarts) and the joins are not free; k_step under the render gains less than that.  Hence off by default; the
// entry point stays: it is the wrapped env's step() as one call.  Only with the fused / in-place consume (a k_consume launch would need
// both halves).
constexpr int64_t STEP_RENDER_SPLIT_MIN = 262144;
#ifndef STEP_RENDER_SPLIT_DEFAULT
#define STEP_RENDER_SPLIT_DEFAULT 0
#endif
// Option "render_delta_from_step" -1 (default): from this batch size up.  BossLevel pixels, bench.py's random actions.  First set to 786 432
// (profiles/render_delta_from_step/): at 1 048 576 envs the render gained more than k_step paid (k_render 608 -> 529 us, k_step 100 -> 143,
// settings alternated in one process: 0.704 -> 0.666 ms per step), while at 131 072 / 262 144 / 524 288 envs k_render_delta's input stage
// was nearly free (82 / 153 / 288 us either way) and k_step paid 11-22 us.  Both sides have moved since: the store-only render is the
// ticketed k_render_dstore_lw, and step_dirty works on four cells per word.  Option 0 against 1 alternated in one process, four repetitions
// each (profiles/step_dirty_packed/ab_from_step_*.jsonl), ms per step: 131 072 envs 0.0964-0.0992 against 0.0958-0.0975 (the ranges
// overlap), 262 144 envs 0.1652-0.1686 against 0.1585-0.1611, 524 288 envs 0.3126-0.3191 against 0.2969-0.3002 (apart, -4 to -5 %).
constexpr int64_t RENDER_FROM_STEP_MIN_ENVS = 262144;
static int step_render_launch_(bbai_env* e, const StepIO& io, uint8_t* pixels, hipStream_t s, bool& dirty) {
    StepPlan p;
    {
        CallScope call(e, s);
        BBAI_TRY(call.rc);
        BBAI_TRY(step_prepare(e, io.auto_reset, s, p));
        // The render is a delta render of the registered target with a valid shadow, and k_step's LDS rows are the step's final observations
        // (fused / in-place consume, or no auto-reset; an unfused k_consume rewrites the finished envs' rows later): k_step finds the dirty
        // cells and updates the shadow (step_dirty), the render only stores (k_render_dstore).  From the step kernel on, the shadow is ahead
        // of the frame until the render has been launched: a failure in between invalidates it (step_render_launch).
        const bool from_step = e->render_delta_from_step < 0 ? e->n >= RENDER_FROM_STEP_MIN_ENVS : e->render_delta_from_step != 0;
        p.dirty = dirty = pixels && from_step && (p.fused || e->inplace || !io.auto_reset) && whole_batch_delta(e->targets.view, (uintptr_t)pixels, e->render_delta != 0);
        const int want = e->step_render_split < 0 ? (STEP_RENDER_SPLIT_DEFAULT && e->n >= STEP_RENDER_SPLIT_MIN) : e->step_render_split;      // (an explicit 1: any size)
        const int64_t nb = step_blocks(e), hb = nb / 2;
        const bool split = want && pixels && (p.fused || !io.auto_reset) && hb > 0;
        if (!split) {
            BBAI_TRY(step_kernel(e, p, io, s, 0, nb));
            BBAI_TRY(step_finish(e, p, io, s));
            BBAI_TRY(call.leave());
            return pixels ? render_launch(e, io.image, pixels, s, -1, 0, p.dirty) : BBAI_OK;
        }
        const int64_t na = hb * STEP_BLOCK;                   // envs of the first half (a multiple of every render group size)
        // the second half's k_step, on the split stream, behind everything the caller's stream holds so far (the gate included)
        HIP_TRY(hipEventRecord(e->ev_split0, s));
        HIP_TRY(hipStreamWaitEvent(e->split, e->ev_split0, 0));
        BBAI_TRY(step_kernel(e, p, io, e->split, hb, nb - hb));
        HIP_TRY(hipEventRecord(e->ev_splitB, e->split));
        BBAI_TRY(step_kernel(e, p, io, s, 0, hb));
        BBAI_TRY(call.leave());
        BBAI_TRY(render_launch(e, io.image, pixels, s, na, 0, p.dirty));
        HIP_TRY(hipStreamWaitEvent(s, e->ev_splitB, 0));
        {
            CallScope call2(e, s);
            BBAI_TRY(call2.rc);
            BBAI_TRY(step_finish(e, p, io, s));
            BBAI_TRY(call2.leave());
        }
        return render_launch(e, io.image + na * OBS_BYTES, pixels + na * (int64_t)PIX_BYTES, s, e->n - na, na, p.dirty);
    }
}
static int step_render_launch(bbai_env* e, const StepIO& io, uint8_t* pixels, hipStream_t s) {
    bool dirty = false;
    const int rc = step_render_launch_(e, io, pixels, s, dirty);
    if (rc != BBAI_OK && dirty) invalidate_target(e->targets.view);       // (a failure before the render's own plan: its commit was never reached)
    return rc;
}

extern "C" {

int bbai_step_render(bbai_env* e, const uint8_t* actions, uint8_t* image, uint8_t* dirs, float* rewards, double* rewards64,
                     uint8_t* dones, int auto_reset, uint8_t* pixels, void* stream) {
    if (!e || !actions || !image || !dirs || !rewards || !dones || !pixels) ARG_FAIL("null handle or buffer");
    BBAI_TRY(step_ready(e, auto_reset, "step"));
    if (e->n_tiles <= 0) { snprintf(g_err, sizeof(g_err), "render before set_atlas"); return BBAI_ERR_STATE; }
    ON_DEVICE(e->device);
    return step_render_launch(e, step_io(e, actions, image, dirs, rewards, rewards64, dones, auto_reset), pixels, (hipStream_t)stream);
}

// Register (or clear with NULL) a caller-owned uint8[n][72] device buffer that the engine keeps filled with the
// mission token ids of every env's current episode (rewritten whenever an env is reset).
int bbai_set_token_buffer(bbai_env* e, uint8_t* tokens_dev) {
    if (!e) ARG_FAIL("null handle");
    e->tokens = tokens_dev;
    if (tokens_dev && e->live) {        // episodes already running: fill every row now
        ON_DEVICE(e->device);
        HIP_TRY(hipDeviceSynchronize());
        hipLaunchKernelGGL(k_tokens, dim3((unsigned)std::min<int64_t>((e->n + 63) / 64, 4096)), dim3(64), 0, 0, e->cfg, e->n, e->rec, e->inplace ? e->next_rec : nullptr, e->depth, e->hot,
                           tokens_dev, e->reset_list, e->counters, 1, nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
    return BBAI_OK;
}

// in-place layout: rec[first ..] <- the live slots (dir 0) or the live slots <- rec[first ..] (dir 1); classic layout: nothing to do
static int live_copy(bbai_env* e, int64_t first, int64_t count, int dir) {
    if (!e->inplace || count <= 0) return BBAI_OK;
    hipLaunchKernelGGL(k_live_copy, dim3((unsigned)std::min<int64_t>((count + 3) / 4, 16384)), dim3(256), 0, 0, e->cfg, e->n, first, count, e->rec,
                       e->next_rec, e->hot, e->depth, dir);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return BBAI_OK;
}

int bbai_export_state(bbai_env* e, int64_t first, int64_t count, uint8_t* rec, uint8_t* hot, uint64_t* stale) {
    if (!e || first < 0 || count < 0 || first + count > e->n) ARG_FAIL("null handle or env range out of bounds");
    ON_DEVICE(e->device);
    HIP_TRY(hipDeviceSynchronize());
    if (rec && count > 0) BBAI_TRY(live_copy(e, first, count, 0));
    if (rec) HIP_TRY(hipMemcpy(rec, e->rec + first * e->cfg.rec_bytes, (size_t)count * e->cfg.rec_bytes, hipMemcpyDeviceToHost));
    if (hot) HIP_TRY(hipMemcpy(hot, e->hot + first, (size_t)count * sizeof(Hot), hipMemcpyDeviceToHost));
    if (stale) HIP_TRY(hipMemcpy(stale, e->stale + first, (size_t)count * 8, hipMemcpyDeviceToHost));
    return BBAI_OK;
}

// window plane + front-cell cache follow the records (they are derived state: not part of exports or checkpoints)
static int sync_view(bbai_env* e, int64_t first, int64_t count) {
    if (e->cplane) {         // (in-place layout: e->rec is the staging area every import / checkpoint load has just filled with the live records)
        hipLaunchKernelGGL(k_sync_cpl, dim3((unsigned)std::min<int64_t>((count + 3) / 4, 16384)), dim3(256), 0, 0, e->cfg, first, count, e->rec, e->hot,
                           e->cplane, e->fcache);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
    if (!e->vplane) return BBAI_OK;
    hipLaunchKernelGGL(k_sync_view, dim3((unsigned)std::min<int64_t>((count + 3) / 4, 16384)), dim3(256), 0, 0, e->cfg, first, count, e->rec, e->hot,
                       e->vplane, e->fcache);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return BBAI_OK;
}

static int import_tokens(bbai_env* e, int64_t first, int64_t count);      // (behind bbai_reseed: it launches k_state_tokens, whose code keeps its place)

int bbai_import_state(bbai_env* e, int64_t first, int64_t count, const uint8_t* rec, const uint8_t* hot, const uint64_t* stale) {
    if (!e || first < 0 || count < 0 || first + count > e->n) ARG_FAIL("null handle or env range out of bounds");
    ON_DEVICE(e->device);
    HIP_TRY(hipDeviceSynchronize());
    if (rec) HIP_TRY(hipMemcpy(e->rec + first * e->cfg.rec_bytes, rec, (size_t)count * e->cfg.rec_bytes, hipMemcpyHostToDevice));
    if (hot && count > 0) {
        // (the imported hot state keeps this env's place in ITS ring in both layouts: the ring belongs to the handle -- in-place, hot.slot
        // says where the live record is; classic, an exporter's slot may not even exist here: it comes from another ring depth)
        Scoped staged;
        BBAI_TRY(staged.mem((size_t)count * sizeof(Hot)));
        HIP_TRY(hipMemcpy(staged.h, hot, (size_t)count * sizeof(Hot), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_import_hot, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, 0, first, count, (Hot*)staged.h, e->hot);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
    if (stale) HIP_TRY(hipMemcpy(e->stale + first, stale, (size_t)count * 8, hipMemcpyHostToDevice));
    if (rec && count > 0) BBAI_TRY(live_copy(e, first, count, 1));
    if (e->lsm && count > 0) HIP_TRY(hipMemset(e->lsm + first, 0, (size_t)count));     // (not part of the exported state: lastStepMatch = False)
    if (rec && count > 0) {
        hipLaunchKernelGGL(k_sync_prog, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, 0, e->cfg, e->n, first, count, e->rec,
                           e->vhead, e->vset);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
    // (a hot / stale-only import: the C plane rows are rebuilt from the staging records, which must then hold the LIVE ones)
    if (!rec && e->cplane && count > 0) BBAI_TRY(live_copy(e, first, count, 0));
    if (count > 0) BBAI_TRY(sync_view(e, first, count));
    if (rec && count > 0) {
        // the expert's plan is not part of an exported state: 0 is no step a plan can expect (k_bot starts a fresh Bot at step 0 anyway), so the
        // env's next decision starts one (k_state_load's rule: BotState::next_step of the range, one strided memset)
        if (e->bot_state) {
            const size_t sbytes = bot_state_bytes(e->bot_stack);
            HIP_TRY(hipMemset2D(e->bot_state + (size_t)first * sbytes + offsetof(BotState, next_step), sbytes, 0, sizeof(uint16_t), (size_t)count));
            HIP_TRY(hipDeviceSynchronize());          // (the import is synchronous: the next bbai_bot_act may come on any stream)
        }
        if (e->tokens) BBAI_TRY(import_tokens(e, first, count));      // (behind the live records and hot states: the sentence k_state_tokens writes)
    }
    e->live = true;
    return BBAI_OK;
}

// ---- checkpoint: EVERYTHING an auto-resetting batch needs to continue bit-identically in another handle --------------
// live records / hot / stale, the MT19937 streams, the look-ahead ring and its window bookkeeping, counters, and the
// expert's plans when the expert has been used.  Blob = header + the device arrays in a fixed order.
struct CkptHeader {
    uint64_t magic; int32_t version, period; int64_t n; LevelCfg cfg; int32_t depth, step_parity, next_counter_clean, seeded, live;
    int32_t has_lsm, pad0, pad1; int32_t bot_stack; int64_t tick; int64_t bot_threads;
};
constexpr int CKPT_VERSION = 4;        // 4: 256-byte next_obs slots (the C plane rows of the small rooms); 3: listless windows (NWIN buffers, meta lines, sharded totals, flow words); 2: env-major look-ahead ring
struct Seg { void* p; size_t bytes; };
// the blob's segments for a handle shaped (period, depth) with / without expert state and done-action bits
static int ckpt_segments(const bbai_env* e, int depth, bool with_bot, int bot_stack, bool with_lsm, Seg* out) {
    const size_t n = (size_t)e->n, D = (size_t)depth, rb = (size_t)e->cfg.rec_bytes;
    int k = 0;
    out[k++] = {e->rec, n * rb}; out[k++] = {e->hot, n * sizeof(Hot)}; out[k++] = {e->stale, n * 8};
    out[k++] = {e->mt, n * MT_N * 4}; out[k++] = {e->mti, n * 4}; out[k++] = {e->vhead, n * 4}; out[k++] = {e->vset, n * 64};
    out[k++] = {e->next_rec, D * n * rb}; out[k++] = {e->next_hot, D * n * sizeof(Hot)};
    out[k++] = {e->pending, NWIN * n}; out[k++] = {e->first_slot, NWIN * n};
    out[k++] = {e->win_meta, NWIN * META_U32 * 4}; out[k++] = {e->totals, SHARDS * SHARD_U64 * 8}; out[k++] = {e->flow, FLOW_WORDS * 8};
    out[k++] = {e->reset_list, n * 4}; out[k++] = {e->counters, 128};
    if (with_bot) { out[k++] = {e->bot_state, n * bot_state_bytes(bot_stack)}; out[k++] = {e->bot_stats, 16}; }
    if (with_lsm) out[k++] = {e->lsm, n};
    if (e->inplace) out[k++] = {e->next_obs, D * n * OBS_SLOT};
    return k;
}

// the lane generator's RNG state <-> the canonical (mts, mtis in [0, 624]) form: both streams idle
static int mt_canon(bbai_env* e) {
    if (!e->mtt) return BBAI_OK;
    hipLaunchKernelGGL(k_mt_canon, dim3((unsigned)((e->n + 3) / 4)), dim3(256), 0, 0, e->n, e->mt, e->mtt, e->mtpar, e->mti);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return BBAI_OK;
}
static int mt_sync(bbai_env* e) {
    if (!e->mtt) return BBAI_OK;
    const int64_t total = e->n * MT_N;
    hipLaunchKernelGGL(k_mt_sync, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, e->n, e->mt, e->mtt, e->mtpar);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return BBAI_OK;
}

int64_t bbai_checkpoint_bytes(bbai_env* e) {
    if (!e) return -1;
    Seg seg[24];
    const int k = ckpt_segments(e, e->depth, e->bot_state != nullptr, e->bot_stack, e->lsm != nullptr, seg);
    size_t total = sizeof(CkptHeader);
    for (int i = 0; i < k; ++i) total += seg[i].bytes;
    return (int64_t)total;
}

int bbai_checkpoint_save(bbai_env* e, void* host_buf, int64_t bytes) {
    if (!e || !host_buf || bytes != bbai_checkpoint_bytes(e)) ARG_FAIL("null pointer or buffer size != bbai_checkpoint_bytes()");
    ON_DEVICE(e->device);
    HIP_TRY(hipDeviceSynchronize());             // both streams idle: the ring and the windows' bookkeeping are at rest, every refill has landed
    BBAI_TRY(live_copy(e, 0, e->n, 0));       // (in-place layout: the blob's record segment = the live slots)
    BBAI_TRY(mt_canon(e));                    // (the blob holds the canonical MT19937 form: every position in [0, 624])
    BBAI_TRY(mt_sync(e));
    CkptHeader h;
    memset(&h, 0, sizeof(h));
    h.magic = 0x42424149434b5054ull; h.version = CKPT_VERSION; h.period = e->period; h.n = e->n; h.cfg = e->cfg; h.depth = e->depth;
    h.step_parity = e->step_parity; h.next_counter_clean = e->next_counter_clean; h.seeded = e->seeded; h.live = e->live;
    h.has_lsm = e->lsm ? 1 : 0;
    h.bot_stack = e->bot_state ? e->bot_stack : 0; h.tick = e->tick; h.bot_threads = e->bot_threads;
    uint8_t* dst = (uint8_t*)host_buf;
    memcpy(dst, &h, sizeof(h)); dst += sizeof(h);
    Seg seg[24];
    const int k = ckpt_segments(e, e->depth, e->bot_state != nullptr, e->bot_stack, e->lsm != nullptr, seg);
    for (int i = 0; i < k; ++i) { HIP_TRY(hipMemcpy(dst, seg[i].p, seg[i].bytes, hipMemcpyDeviceToHost)); dst += seg[i].bytes; }
    return BBAI_OK;
}

static int bot_alloc(bbai_env* e, int cap);

int bbai_checkpoint_load(bbai_env* e, const void* host_buf, int64_t bytes) {
    if (!e || !host_buf || bytes < (int64_t)sizeof(CkptHeader)) ARG_FAIL("null pointer or short buffer");
    CkptHeader h;
    memcpy(&h, host_buf, sizeof(h));
    if (h.magic != 0x42424149434b5054ull) ARG_FAIL("not a bbai checkpoint");
    if (h.version != CKPT_VERSION) {
        snprintf(g_err, sizeof(g_err), "bbai_checkpoint_load: unsupported checkpoint version %d (this library reads version %d)", h.version, CKPT_VERSION);
        return BBAI_ERR_ARG;
    }
    if (h.n != e->n || memcmp(&h.cfg, &e->cfg, sizeof(LevelCfg)) != 0 || h.period < 1 || h.period > MAX_PERIOD || h.depth != 2 * h.period + e->inplace)
        ARG_FAIL("checkpoint was taken from a different level / batch size / state layout (BBAI_INPLACE)");
    // EVERYTHING is validated before the handle is touched (a refused blob leaves the handle exactly as it was): the expert's stack
    // capacity, the done-action mode, and the blob's size for the shape its header announces.
    if (h.bot_stack && e->bot_state && e->bot_stack != h.bot_stack) ARG_FAIL("the handle's expert uses a different stack capacity (BBAI_BOT_STACK)");
    if ((h.has_lsm != 0) != (e->lsm != nullptr)) ARG_FAIL("checkpoint and handle differ in the done-action mode (bbai_set_done_actions)");
    {
        Seg seg[24];
        const int k = ckpt_segments(e, h.depth, h.bot_stack != 0, h.bot_stack, h.has_lsm != 0, seg);
        size_t total = sizeof(CkptHeader);
        for (int i = 0; i < k; ++i) total += seg[i].bytes;
        if ((int64_t)total != bytes) ARG_FAIL("checkpoint size does not match its header (truncated blob?)");
    }
    ON_DEVICE(e->device);
    HIP_TRY(hipDeviceSynchronize());
    if (h.bot_stack && !e->bot_state) {          // (allocates only; on failure the handle is unchanged)
        BBAI_TRY(bot_alloc(e, h.bot_stack));
    }
    if (h.period != e->period) {
        // The handle chose its look-ahead period from the memory that was free when it was created (bbai_create); the blob's
        // ring has the saving handle's.  The ring is part of the state: take the blob's shape.  The new ring is allocated BEFORE the
        // old one is let go, so that a failure leaves the handle as it was.
        Ring r;
        if (ring_alloc(e, h.depth, r) != BBAI_OK) {
            snprintf(g_err, sizeof(g_err), "checkpoint_load: no memory for the checkpoint's look-ahead ring (period %d); the handle is unchanged", h.period);
            return BBAI_ERR_NOMEM;
        }
        ring_install(e, r, h.period);
    }
    const bool had_bot = e->bot_state != nullptr;
    if (!h.bot_stack && had_bot) {               // checkpoint without expert state: every env gets a fresh Bot
        HIP_TRY(hipMemset(e->bot_state, 0, (size_t)e->n * bot_state_bytes(e->bot_stack)));
        HIP_TRY(hipMemset(e->bot_stats, 0, 16));
    }
    Seg seg[24];
    const int k = ckpt_segments(e, e->depth, h.bot_stack != 0, h.bot_stack, h.has_lsm != 0, seg);
    const uint8_t* src = (const uint8_t*)host_buf + sizeof(CkptHeader);
    // (from here on a failing copy leaves a half-loaded handle: it must not be stepped)
    e->seeded = e->live = false;
    for (int i = 0; i < k; ++i) { HIP_TRY(hipMemcpy(seg[i].p, src, seg[i].bytes, hipMemcpyHostToDevice)); src += seg[i].bytes; }
    e->step_parity = h.step_parity; e->next_counter_clean = h.next_counter_clean != 0; e->seeded = h.seeded != 0; e->live = h.live != 0;
    e->tick = h.tick;
    // (the saved run was idle: every refill it had launched has landed, and flow[FLOW_REFILLED] in the blob says so)
    for (int i = 0; i < NWIN; ++i) HIP_TRY(hipEventRecord(e->ev_refill[i], e->side));
    HIP_TRY(hipDeviceSynchronize());
    BBAI_TRY(mt_sync(e));
    return sync_view(e, 0, e->n);
}

int bbai_get_programs(bbai_env* e, int64_t first, int64_t count, uint8_t* prog) {
    if (!e || !prog || first < 0 || count < 0 || first + count > e->n) ARG_FAIL("null pointer or env range out of bounds");
    ON_DEVICE(e->device);
    HIP_TRY(hipDeviceSynchronize());
    BBAI_TRY(live_copy(e, first, count, 0));
    HIP_TRY(hipMemcpy2D(prog, sizeof(Prog), e->rec + first * e->cfg.rec_bytes + e->cfg.off_prog, (size_t)e->cfg.rec_bytes,
                        sizeof(Prog), (size_t)count, hipMemcpyDeviceToHost));
    return BBAI_OK;
}

static int bot_alloc(bbai_env* e, int cap) {             // the expert's state: all four buffers or none
    const int64_t threads = std::min<int64_t>((e->n + 63) / 64 * 64, 256 * 8 * 64);
    Scoped st, wk, rw, ss;
    const size_t sbytes = bot_state_bytes(cap);
    int rc = st.mem((size_t)e->n * sbytes);
    if (rc == BBAI_OK) rc = wk.mem((size_t)threads * BOT_WORK_WORDS * sizeof(uint16_t));
    if (rc == BBAI_OK) rc = rw.mem((size_t)threads * (R_ALL - R_FAST) * MAX_W * sizeof(uint32_t));
    if (rc == BBAI_OK) rc = ss.mem(16);
    if (rc == BBAI_OK) rc = res_done("hipMemset", hipMemset(st.h, 0, (size_t)e->n * sbytes));
    if (rc == BBAI_OK) rc = res_done("hipMemset", hipMemset(ss.h, 0, 16));
    if (rc != BBAI_OK) {
        snprintf(g_err, sizeof(g_err), "allocating the expert's state failed: %s", hipGetErrorString(g_hip));
        return BBAI_ERR_NOMEM;
    }
    e->bot_stack = cap;
    e->own.adopt(&e->bot_state, st); e->own.adopt(&e->bot_work, wk); e->own.adopt(&e->bot_stats, ss); e->bot_threads = threads;
    e->own.adopt(&e->bot_rows, rw);
    { const char* ev = getenv("BBAI_BOT_EAGER"); e->bot_eager = ev ? atoi(ev) != 0 : 1; }
    return BBAI_OK;
}

// k_bot on stream s (allocates the expert's state on first use); the caller has entered the call
static int bot_launch(bbai_env* e, const uint8_t* prev_actions, uint8_t* actions, int dead_action, uint8_t* gave_up, hipStream_t s) {
    if (!e->bot_state) {                                   // first use
        // Subgoal stack depth per env.  The reference's list is unbounded; 48 covers every plan that makes progress (the
        // rare bot that loops without progress grows its stack until max_steps and fails the episode -- here it gives up
        // when the stack is full, counted in bbai_bot_stats().capacity).  Raise it to follow such a bot further.
        const char* ev = getenv("BBAI_BOT_STACK");
        BBAI_TRY(bot_alloc(e, ev ? std::max(8, std::min(atoi(ev), 4096)) : BOT_STACK));
    }
    // Occupancy target, measured (profiles/r01/bot_bench.jsonl): the fully inlined expert wants ~400
    // registers; capping it at 256 (2 waves/SIMD, spills to scratch) is +35 % on maze levels (BossLevel 1M envs 22.8 ->
    // 17.0 ms) and -10 % on single rooms, 128 registers (4 waves/SIMD) loses everywhere, real calls instead of inlining too.
    const bool maze = e->cfg.num_rows * e->cfg.num_cols > 1;
    unsigned long long* stats = (unsigned long long*)e->bot_stats;
#if !BBAI_BOT_GROUP_BUILD
    if (e->bot_group) { snprintf(g_err, sizeof(g_err), "this library was built without the lane-group expert (k_botg: an experiment build, -DBBAI_BOT_GROUP_BUILD=1)"); return BBAI_ERR_ARG; }
#else
    if (e->bot_group) {                                     // one lane group per env (k_botg)
        // Measured (profiles/r05/NOTES.md section 11): same decisions, 1.9-2.4 x SLOWER than lane = env -- a group executes 3.4 x the
        // instructions per env (the subgoal machine runs redundantly on the group's lanes, 4 envs share a wave's issue slots instead
        // of 64) and only gets 1.8 x the instructions per cycle back.  Kept as an option for experiments, off by default.
        constexpr int G = 16;
        if (e->bot_group != G) { snprintf(g_err, sizeof(g_err), "no k_botg build for %d lanes per env (only 16)", e->bot_group); return BBAI_ERR_ARG; }
        const int64_t threads = std::min<int64_t>((e->n * G + 63) / 64 * 64, (int64_t)256 * 8 * 64);
        const size_t glds = (size_t)(64 / G) * botg_group_words(e->cfg) * 4;     // BossLevel: 4 x 2.5 KB
        hipLaunchKernelGGL((k_botg<G, 2>), dim3((unsigned)(threads / 64)), dim3(64), glds, s, e->cfg, e->n, e->rec, e->inplace ? e->next_rec : nullptr, e->depth, e->hot,
                           e->stale, e->bot_state, e->bot_stack, e->bot_work, e->bot_eager, prev_actions, actions, stats, dead_action, gave_up);
        HIP_TRY(hipGetLastError());
        return BBAI_OK;
    }
#endif
    const dim3 grid((unsigned)(e->bot_threads / 64)), block(64);
    const size_t lds = (size_t)R_FAST * e->cfg.H * 64 * 4 + (size_t)BOT_RING * 64 * 2;     // BossLevel: 11.3 + 8 KB -> 8 waves per CU
    // ONE instantiation for every geometry: round 5's packed lists took the kernel from ~400 wanted registers to a shape that fits 256 with 24 spilled, and
    // the single rooms then prefer two waves per SIMD as well (profiles/r05/bot_round5_experiments.jsonl: PickupLoc 262 144 1.09 -> 0.95 ms per decision + step,
    // GoToLocal 65 536 0.357 -> 0.353); round 1's k_bot<1> for them is gone.
    (void)maze;
    hipLaunchKernelGGL(k_bot<2>, grid, block, lds, s, e->cfg, e->n, e->rec, e->inplace ? e->next_rec : nullptr, e->depth, e->hot, e->stale, e->bot_state, e->bot_stack, e->bot_work,
                       e->bot_rows, e->bot_eager, prev_actions, actions, stats, dead_action, gave_up);
    HIP_TRY(hipGetLastError());
    return BBAI_OK;
}

int bbai_bot_act(bbai_env* e, const uint8_t* prev_actions, uint8_t* actions, void* stream) {
    if (!e || !actions) ARG_FAIL("null handle or output buffer");
    if (!e->live) { snprintf(g_err, sizeof(g_err), "bot_act before reset"); return BBAI_ERR_STATE; }
    ON_DEVICE(e->device);
    hipStream_t s = (hipStream_t)stream;
    CallScope call(e, s);
    BBAI_TRY(call.rc);
    BBAI_TRY(bot_launch(e, prev_actions, actions, BOT_DEAD, nullptr, s));
    return call.leave();
}

// T expert decisions + steps with no host round trip in between (the inner loop of generate_demos).
int bbai_bot_rollout(bbai_env* e, int T, uint8_t* image, uint8_t* dirs, uint8_t* images_out, uint8_t* dirs_out, uint8_t* tokens_out,
                     uint8_t* actions_out, float* rewards_out, uint8_t* dones_out, uint8_t* gave_up_out, void* stream) {
    if (!e || T < 1 || !image || !dirs || !images_out || !dirs_out || !actions_out || !rewards_out || !dones_out || !gave_up_out)
        ARG_FAIL("null handle or buffer, or T < 1");
    if (!e->live || !e->seeded) { snprintf(g_err, sizeof(g_err), "bot_rollout before seed + reset"); return BBAI_ERR_STATE; }
    if (tokens_out && !e->tokens) { snprintf(g_err, sizeof(g_err), "bot_rollout: tokens_out needs a registered token buffer (bbai_set_token_buffer)"); return BBAI_ERR_STATE; }
    ON_DEVICE(e->device);
    hipStream_t s = (hipStream_t)stream;
    CallScope call(e, s);
    BBAI_TRY(call.rc);
    const size_t n = (size_t)e->n;
    for (int t = 0; t < T; ++t) {
        // what the expert decides on: the observation (and mission) BEFORE the step
        HIP_TRY(hipMemcpyAsync(images_out + (size_t)t * n * OBS_BYTES, image, n * OBS_BYTES, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(dirs_out + (size_t)t * n, dirs, n, hipMemcpyDeviceToDevice, s));
        if (tokens_out) HIP_TRY(hipMemcpyAsync(tokens_out + (size_t)t * n * TOK_MAX, e->tokens, n * TOK_MAX, hipMemcpyDeviceToDevice, s));
        BBAI_TRY(bot_launch(e, nullptr, actions_out + (size_t)t * n, A_RESET_ENV, gave_up_out + (size_t)t * n, s));
        BBAI_TRY(step_launch(e, StepIO{actions_out + (size_t)t * n, image, dirs, rewards_out + (size_t)t * n, nullptr, dones_out + (size_t)t * n, 1,
                                       1 /* the expert's `done` is the enum member (bot.py:593) */, -1 /* ... and it never holds */}, s));
    }
    return call.leave();
}

#if defined(BBAI_BOT_PROF)
int bbai_bot_prof_read(unsigned long long* out32, int reset) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_bot_prof), 32 * 8));
    if (reset) { unsigned long long z[32] = {}; HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_bot_prof), z, sizeof(z))); }
    return BBAI_OK;
}
#endif

int bbai_bot_stats(bbai_env* e, uint64_t* gave_up, uint64_t* capacity) {
    if (!e || !gave_up || !capacity) ARG_FAIL("null pointer");
    ON_DEVICE(e->device);
    *gave_up = *capacity = 0;
    if (!e->bot_stats) return BBAI_OK;
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long v[2] = {0, 0};
    HIP_TRY(hipMemcpy(v, e->bot_stats, 16, hipMemcpyDeviceToHost));
    *gave_up = v[0]; *capacity = v[1];
    return BBAI_OK;
}

static int tap_launch(int64_t count, int64_t pix_count, const int64_t* ids, const uint8_t* image, const uint8_t* dirs, const double* rew64,
                      const uint8_t* dones, const uint8_t* pixels, uint8_t* image_out, uint8_t* dirs_out, double* rew64_out, uint8_t* dones_out,
                      uint8_t* pixels_out, void* stream) {
    if (count <= 0 || pix_count < 0 || pix_count > count || !image || !dirs || !rew64 || !dones || !image_out || !dirs_out || !rew64_out || !dones_out ||
        (pix_count && (!pixels || !pixels_out || ((uintptr_t)pixels & 15) || ((uintptr_t)pixels_out & 15))))
        ARG_FAIL("null / misaligned pointer or empty tap");
    const int64_t work = std::max<int64_t>(count * OBS_BYTES, pix_count * (PIX_BYTES / 16));
    hipLaunchKernelGGL(k_tap, dim3((unsigned)std::min<int64_t>((work + 255) / 256, 2048)), dim3(256), 0, (hipStream_t)stream, count, pix_count, ids,
                       image, dirs, rew64, dones, pixels, image_out, dirs_out, rew64_out, dones_out, pixels_out);
    HIP_TRY(hipGetLastError());
    return BBAI_OK;
}

int bbai_tap(int64_t count, int64_t pix_count, const uint8_t* image, const uint8_t* dirs, const double* rew64, const uint8_t* dones,
             const uint8_t* pixels, uint8_t* image_out, uint8_t* dirs_out, double* rew64_out, uint8_t* dones_out, uint8_t* pixels_out,
             void* stream) {
    return tap_launch(count, pix_count, nullptr, image, dirs, rew64, dones, pixels, image_out, dirs_out, rew64_out, dones_out, pixels_out, stream);
}

int bbai_tap_ids(int64_t count, int64_t pix_count, const int64_t* ids_dev, const uint8_t* image, const uint8_t* dirs, const double* rew64,
                 const uint8_t* dones, const uint8_t* pixels, uint8_t* image_out, uint8_t* dirs_out, double* rew64_out, uint8_t* dones_out,
                 uint8_t* pixels_out, void* stream) {
    if (!ids_dev) ARG_FAIL("null id list");
    return tap_launch(count, pix_count, ids_dev, image, dirs, rew64, dones, pixels, image_out, dirs_out, rew64_out, dones_out, pixels_out, stream);
}

// T steps of the hot path with no host round trip in between (include/bbai.h): what a caller's loop of bbai_step [+ bbai_render]
// [+ bbai_tap_ids] enqueues, enqueued from here.  (Built on the suspicion that an interpreter's per-step overhead does not stay
// ahead of a 40-us step -- a rocprofv3 trace shows 10-us gaps between the kernels of one step, profiles/r04/kernel_trace_gaps_*.txt --
// and measured equal to the Python loop on every config: the gaps are the tracer's.  Kept as the open-loop entry it is.)
int bbai_rollout(bbai_env* e, int T, const uint8_t* actions, uint8_t* image, uint8_t* dirs, float* rewards, double* rewards64, uint8_t* dones,
                 int auto_reset, uint8_t* pixels, const bbai_tap_log* tap, void* stream) {
    if (!e || T < 1 || !actions || !image || !dirs || !rewards || !dones) ARG_FAIL("null handle or buffer, or T < 1");
    BBAI_TRY(step_ready(e, auto_reset, "rollout"));
    if (pixels && e->n_tiles <= 0) { snprintf(g_err, sizeof(g_err), "rollout with pixels before set_atlas"); return BBAI_ERR_STATE; }
    if (tap && (!rewards64 || tap->count <= 0 || tap->pix_count < 0 || tap->pix_count > tap->count || !tap->image_out || !tap->dir_out ||
                !tap->reward64_out || !tap->done_out || (tap->pix_count && (!pixels || !tap->pixels_out))))
        ARG_FAIL("tap log incomplete (it needs reward64_dev, and pixels_dev for its pixel rows)");
    ON_DEVICE(e->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)e->n;
    const bool own_tap = tap && !tap->ids_dev;          // the envs of bbai_step_tap_set, logged by the stepping lanes
    StepIO io = step_io(e, actions, image, dirs, rewards, rewards64, dones, auto_reset);
    auto tap_rows = [&](int t) {                        // the tap log's rows of tick t
        const size_t c = (size_t)tap->count, orow = (size_t)(tap->obs_row0 + t), row = (size_t)(tap->row0 + t);
        return TapRows{tap->image_out + orow * c * OBS_BYTES, tap->dir_out + orow * c, tap->reward64_out + row * c, tap->done_out + row * c};
    };
    if (own_tap && (tap->count != e->tap_count || tap->pix_count != 0)) {
        snprintf(g_err, sizeof(g_err), "rollout: a tap log without ids_dev follows bbai_step_tap_set's list (%lld envs, no pixel rows)", (long long)e->tap_count);
        return BBAI_ERR_ARG;
    }
    // Encoded observations, the finished envs moved on inside k_step (or nobody resets): the launches carry as many ticks as the look-ahead
    // window has left -- the same bytes as tick-by-tick launches (tests/test_gpu_parity.py::test_rollout_*), without their boundaries.
    // An unfused auto-reset (k_consume between the steps), a token buffer (k_tokens reads every step's dones) or a tap that is a launch
    // keep one step per launch.
    const bool fused = auto_reset && (e->inplace || use_fused_consume(e));
    if (!pixels && (fused || !auto_reset) && !e->tokens && (!tap || own_tap) && (e->rollout_multi || own_tap)) {
        CallScope call(e, s);
        BBAI_TRY(call.rc);
        for (int t = 0; t < T;) {
            StepPlan p;
            BBAI_TRY(step_prepare(e, auto_reset, s, p));
            int ticks = e->rollout_multi ? T - t : 1;
            if (fused) ticks = std::min(ticks, e->period - tick_pos(e).pos);
            if (own_tap) p.tap = tap_args(e, tap_rows(t));         // (tap->count == e->tap_count: checked above)
            io.actions = actions + (size_t)t * n;
            BBAI_TRY(step_kernel(e, p, io, s, 0, step_blocks(e), ticks));
            if (fused) BBAI_TRY(window_end(e, s, 2, dones, ticks));
            t += ticks;
        }
        return call.leave();
    }
    if (own_tap && pixels) { snprintf(g_err, sizeof(g_err), "rollout: a tap log without ids_dev has no pixel rows (encoded observations only)"); return BBAI_ERR_ARG; }
    for (int t = 0; t < T; ++t) {
        io.actions = actions + (size_t)t * n;
        const TapRows rows = tap ? tap_rows(t) : TapRows{};
        if (own_tap) {          // (unfused auto-reset / a token buffer: one bbai_step_tapped per step)
            CallScope call(e, s);
            BBAI_TRY(call.rc);
            BBAI_TRY(step_launch(e, io, s, &rows));
            BBAI_TRY(call.leave());
            continue;
        }
        BBAI_TRY(step_render_launch(e, io, pixels, s));
        if (tap) BBAI_TRY(tap_launch(tap->count, tap->pix_count, tap->ids_dev, image, dirs, rewards64, dones, pixels, rows.image_out, rows.dir_out, rows.rew_out, rows.done_out,
                                     tap->pix_count ? tap->pixels_out + (size_t)(tap->obs_row0 + t) * (size_t)tap->pix_count * PIX_BYTES : nullptr, stream));
    }
    return BBAI_OK;
}

int bbai_gae(int64_t num_envs, int num_frames, const float* rewards, const float* values, const float* masks, const float* last_mask,
             const float* last_value, double discount, double gae_lambda, float* advantage, float* returnn, void* stream) {
    if (num_envs <= 0 || num_frames <= 0 || !rewards || !values || !masks || !last_mask || !last_value || !advantage || !returnn)
        ARG_FAIL("null pointer or empty rollout");
    hipLaunchKernelGGL(k_gae, dim3((unsigned)((num_envs + 63) / 64)), dim3(64), 0, (hipStream_t)stream, num_envs, num_frames, rewards, values,
                       masks, last_mask, last_value, (float)discount, (float)(discount * gae_lambda), advantage, returnn);
    HIP_TRY(hipGetLastError());
    return BBAI_OK;
}

// The entries of the demo store (bbai_demo.hpp): handle-free like bbai_gae, launched on the current device.
static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

int bbai_demo_spans(int64_t n, int chunk, const uint8_t* done, const uint8_t* gave_up, const float* reward, int64_t g0, int filter_steps,
                    int32_t* last_done, uint8_t* open, int32_t* span, uint64_t* open_count, void* stream) {
    if (n <= 0 || chunk <= 0 || !done || !gave_up || !reward || !last_done || !open || !span || !open_count) ARG_FAIL("null pointer or empty chunk");
    if (g0 < 0 || g0 + chunk > 0x7fffffff || filter_steps < 0) ARG_FAIL("step index out of range");
    HIP_TRY(hipMemsetAsync(open_count, 0, sizeof(uint64_t), (hipStream_t)stream));
    hipLaunchKernelGGL(k_demo_spans, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, n, chunk, done, gave_up, reward, (int)g0,
                       filter_steps, last_done, open, span, (unsigned long long*)open_count);
    HIP_TRY(hipGetLastError());
    return BBAI_OK;
}

int bbai_demo_pack(int64_t n, int64_t frames, int chunk_steps, const bbai_demo_chunk* chunks, const int32_t* span, const int64_t* offset,
                   uint8_t* image_out, uint8_t* dir_out, uint8_t* action_out, uint8_t* tokens_out, void* stream) {
    if (n <= 0 || frames < n || chunk_steps <= 0 || !chunks || !span || !offset || !image_out || !dir_out || !action_out || !tokens_out)
        ARG_FAIL("null pointer or empty store");
    if (!aligned16(image_out) || !aligned16(dir_out) || !aligned16(action_out) || !aligned16(tokens_out)) ARG_FAIL("outputs must be 16-byte aligned");
    static_assert(sizeof(bbai_demo_chunk) == sizeof(DemoChunkPtrs), "bbai_demo_chunk");
    DemoPackArgs a;
    a.n = n; a.frames = frames; a.T = chunk_steps;
    a.img_blocks = (frames * (int64_t)DEMO_ROW + DEMO_BLOCK_BYTES - 1) / DEMO_BLOCK_BYTES;
    a.meta_blocks = ((frames + 3) / 4 + DEMO_BLOCK - 1) / DEMO_BLOCK;
    const int64_t tok_blocks = (n * 9 + DEMO_BLOCK - 1) / DEMO_BLOCK;
    a.chunks = (const DemoChunkPtrs*)chunks; a.span = span; a.offset = offset;
    a.image = image_out; a.dir = dir_out; a.action = action_out; a.tokens = tokens_out;
    if (a.img_blocks + a.meta_blocks + tok_blocks > 0x7fffffff) ARG_FAIL("store too large for one launch");
    hipLaunchKernelGGL(k_demo_pack, dim3((unsigned)(a.img_blocks + a.meta_blocks + tok_blocks)), dim3(DEMO_BLOCK), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return BBAI_OK;
}

int bbai_demo_jobs(int64_t n, int chunk, const uint8_t* done, const uint8_t* gave_up, const float* reward, int64_t g0, int32_t* job, int32_t* start,
                   const uint64_t* job_seeds, int64_t n_jobs, int64_t* ids_out, uint64_t* seeds_out, int32_t* records_out, uint64_t* counters,
                   void* stream) {
    if (n <= 0 || chunk <= 0 || !done || !gave_up || !reward || !job || !start || !job_seeds || !ids_out || !seeds_out || !records_out || !counters)
        ARG_FAIL("null pointer or empty chunk");
    if (g0 < 0 || g0 + chunk > 0x7fffffff || n_jobs < 0 || n_jobs > 0x7fffffff) ARG_FAIL("step index or job count out of range");
    HIP_TRY(hipMemsetAsync(counters + 2, 0, 2 * sizeof(uint64_t), (hipStream_t)stream));
    hipLaunchKernelGGL(k_demo_jobs, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, n, chunk, done, gave_up, reward, (int)g0, job, start,
                       job_seeds, n_jobs, ids_out, seeds_out, records_out, (unsigned long long*)counters);
    HIP_TRY(hipGetLastError());
    return BBAI_OK;
}

int bbai_demo_pack_list(int64_t count, int64_t frames, int64_t n_streams, int chunk_steps, int ring_slots, const bbai_demo_chunk* chunks,
                        const int32_t* records, const int64_t* offset, uint8_t* image_out, uint8_t* dir_out, uint8_t* action_out, uint8_t* tokens_out,
                        void* stream) {
    if (count <= 0 || frames < count || n_streams <= 0 || chunk_steps <= 0 || ring_slots <= 0 || !chunks || !records || !offset || !image_out || !dir_out ||
        !action_out || !tokens_out) ARG_FAIL("null pointer or empty list");
    if (!aligned16(image_out) || !aligned16(dir_out) || !aligned16(action_out) || !aligned16(tokens_out)) ARG_FAIL("outputs must be 16-byte aligned");
    DemoPackListArgs a;
    a.n = count; a.frames = frames; a.T = chunk_steps; a.n_streams = n_streams; a.R = ring_slots;
    a.img_blocks = (frames * (int64_t)DEMO_ROW + DEMO_BLOCK_BYTES - 1) / DEMO_BLOCK_BYTES;
    a.meta_blocks = ((frames + 3) / 4 + DEMO_BLOCK - 1) / DEMO_BLOCK;
    const int64_t tok_blocks = (count * 9 + DEMO_BLOCK - 1) / DEMO_BLOCK;
    a.chunks = (const DemoChunkPtrs*)chunks; a.rec = records; a.offset = offset;
    a.image = image_out; a.dir = dir_out; a.action = action_out; a.tokens = tokens_out;
    if (a.img_blocks + a.meta_blocks + tok_blocks > 0x7fffffff) ARG_FAIL("list too large for one launch");
    hipLaunchKernelGGL(k_demo_pack_list, dim3((unsigned)(a.img_blocks + a.meta_blocks + tok_blocks)), dim3(DEMO_BLOCK), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return BBAI_OK;
}

// The replay entries (include/bbai_demo_replay.h): one tick of a pool that plays a store back = feed, bbai_step, judge.
int bbai_demo_replay_feed(int64_t n, const uint8_t* image, const uint8_t* dir, const uint8_t* tokens, const int32_t* job, const int32_t* pos,
                          int64_t n_demos, int64_t frames, const int64_t* offset, const uint8_t* store_image, const uint8_t* store_dir,
                          const uint8_t* store_action, const uint8_t* store_tokens, int32_t* mismatches, int32_t* first_mismatch, uint8_t* mission_ok,
                          uint8_t* actions_out, uint8_t* fed_out, void* stream) {
    if (n < 0 || n > 0x7fffffff || n_demos < 1 || n_demos > 0x7fffffff || frames < 1) ARG_FAIL("pool, demo or frame count out of range");
    if (n == 0) return BBAI_OK;
    if (!image || !dir || !tokens || !job || !pos || !offset || !store_image || !store_dir || !store_action || !store_tokens || !mismatches ||
        !first_mismatch || !mission_ok || !actions_out || !fed_out) ARG_FAIL("null pointer");
    if (!aligned16(image) || !aligned16(store_image)) ARG_FAIL("image arrays must be 16-byte aligned");
    if (((uintptr_t)tokens | (uintptr_t)store_tokens) & 7u) ARG_FAIL("token rows must be 8-byte aligned");
    DemoReplayFeedArgs a;
    a.n = n; a.n_demos = n_demos; a.frames = frames;
    a.image = image; a.dir = dir; a.tokens = tokens; a.job = job; a.pos = pos; a.offset = offset;
    a.s_image = store_image; a.s_dir = store_dir; a.s_action = store_action; a.s_tokens = store_tokens;
    a.mismatches = mismatches; a.first_mismatch = first_mismatch; a.mission_ok = mission_ok; a.actions_out = actions_out; a.fed = fed_out;
    hipLaunchKernelGGL(k_demo_replay_feed, dim3((unsigned)((n + REPLAY_ENVS - 1) / REPLAY_ENVS)), dim3(DEMO_BLOCK), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return BBAI_OK;
}

int bbai_demo_replay_judge(int64_t n, const uint8_t* fed, const uint8_t* done, const double* reward64, int32_t* job, int32_t* pos, int64_t n_demos,
                           const int64_t* offset, int32_t* played, int32_t* done_at, double* return64, int claim, const int32_t* job_demo,
                           const uint64_t* job_seeds, int64_t n_jobs, int64_t* ids_out, uint64_t* seeds_out, uint64_t* counters, void* stream) {
    if (n < 0 || n > 0x7fffffff || n_demos < 1 || n_demos > 0x7fffffff || n_jobs < 0 || n_jobs > 0x7fffffff)
        ARG_FAIL("pool, demo or job count out of range");
    if (n == 0) return BBAI_OK;
    if (!fed || !done || !reward64 || !job || !pos || !offset || !played || !done_at || !return64 || !counters) ARG_FAIL("null pointer");
    if (claim && (!ids_out || !seeds_out || (n_jobs && !job_seeds))) ARG_FAIL("a claim needs ids_out, seeds_out and the job list");
    DemoReplayJudgeArgs a;
    a.n = n; a.n_demos = n_demos; a.n_jobs = n_jobs; a.claim = claim;
    a.fed = fed; a.done = done; a.reward64 = reward64; a.job = job; a.pos = pos; a.offset = offset;
    a.played = played; a.done_at = done_at; a.return64 = return64; a.job_demo = job_demo; a.job_seeds = job_seeds;
    a.ids_out = ids_out; a.seeds_out = seeds_out; a.counters = (unsigned long long*)counters;
    hipLaunchKernelGGL(k_demo_replay_judge, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return BBAI_OK;
}

int bbai_demo_batch(int64_t count, int64_t frames, const int64_t* order, const int64_t* dst_start, const int64_t* offset, const uint8_t* src_image,
                    const uint8_t* src_dir, const uint8_t* src_action, uint8_t* image_out, int64_t* action_out, uint8_t* done_out, float* mask_out,
                    int64_t* episode_ids_out, uint8_t* dir8_out, uint8_t* action8_out, void* stream) {
    if (count <= 0 || frames < count || !order || !dst_start || !offset || !src_image || !src_action || !image_out) ARG_FAIL("null pointer or empty batch");
    const bool batch_form = action_out && done_out && mask_out && episode_ids_out && !dir8_out && !action8_out;
    const bool store_form = !action_out && !done_out && !mask_out && !episode_ids_out && dir8_out && action8_out && src_dir;
    if (!batch_form && !store_form) ARG_FAIL("pass either action / done / mask / episode_ids or dir8 / action8 (with src_dir)");
    if (!aligned16(src_image) || !aligned16(image_out) || !aligned16(action_out) || !aligned16(done_out) || !aligned16(mask_out) ||
        !aligned16(episode_ids_out) || !aligned16(dir8_out) || !aligned16(action8_out)) ARG_FAIL("src_image and the outputs must be 16-byte aligned");
    DemoBatchArgs a;
    a.B = count; a.frames = frames;
    a.img_blocks = (frames * (int64_t)DEMO_ROW + DEMO_BLOCK_BYTES - 1) / DEMO_BLOCK_BYTES;
    const int64_t meta_blocks = ((frames + 3) / 4 + DEMO_BLOCK - 1) / DEMO_BLOCK;
    a.order = order; a.dst_start = dst_start; a.offset = offset; a.src_image = src_image; a.src_dir = src_dir; a.src_action = src_action;
    a.image = image_out; a.action64 = action_out; a.done = done_out; a.mask = mask_out; a.episode = episode_ids_out; a.dir8 = dir8_out; a.action8 = action8_out;
    if (a.img_blocks + meta_blocks > 0x7fffffff) ARG_FAIL("batch too large for one launch");
    hipLaunchKernelGGL(k_demo_batch, dim3((unsigned)(a.img_blocks + meta_blocks)), dim3(DEMO_BLOCK), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return BBAI_OK;
}

int bbai_set_call_events(bbai_env* e, int enable) {
    if (!e) ARG_FAIL("null handle");
    if (enable && !e->call_events && e->have_stream) {      // switching on mid-run: the event must describe the work so far
        ON_DEVICE(e->device);
        HIP_TRY(hipEventRecord(e->ev_switch, e->last_stream));
    }
    e->call_events = enable != 0;
    return BBAI_OK;
}


// The reference's BABYAI_DONE_ACTIONS verifier mode for this handle (on by default iff that variable was non-empty at
// bbai_create, as the reference reads it at import).  Switching it resets every env's lastStepMatch bits.
int bbai_set_done_actions(bbai_env* e, int enable) {
    if (!e) ARG_FAIL("null handle");
    ON_DEVICE(e->device);
    HIP_TRY(hipDeviceSynchronize());
    if (enable && !e->lsm) BBAI_TRY(e->own.alloc({{&e->lsm, (size_t)e->n}}));
    if (!enable) BBAI_TRY(e->own.drop(&e->lsm));
    if (e->lsm) HIP_TRY(hipMemset(e->lsm, 0, (size_t)e->n));
    return BBAI_OK;
}
int bbai_get_done_actions(bbai_env* e) { return e && e->lsm ? 1 : 0; }

// Performance knobs by name (KNOBS, plus the three that do work): what the BBAI_* environment variables set at bbai_create, switchable on a
// live handle so that measurements can alternate settings inside ONE process on ONE box (tools/ab.py).  Synchronises the device first
// ("reseed_levels" and "step_hold" aside: a caller sets them around single bbai_reseed / stepping calls of a running loop).
int bbai_set_option(bbai_env* e, const char* name, int64_t value) {
    if (!e || !name) ARG_FAIL("null handle or name");
    ON_DEVICE(e->device);
    const Knob* k = find_knob(name);
    // (a bbai_reseed reads its depth, a stepping call its hold byte, on the host when it is enqueued: nothing in flight sees either)
    if (!(k && (k->field == &bbai_env::reseed_levels || k->field == &bbai_env::step_hold))) HIP_TRY(hipDeviceSynchronize());
    const int v = (int)value;
    if (!strcmp(name, "pregen_lane")) {
        if (!e->mtt) { if (v) ARG_FAIL("pregen_lane: this level kind / layout is not covered by the lane generator"); }
        else if ((v != 0) != (e->pregen_lane != 0)) {
            HIP_TRY(hipDeviceSynchronize());
            // the lane-group kernel reads and writes the canonical form; the lane kernel needs the tempered halves behind it
            BBAI_TRY(mt_canon(e));
            BBAI_TRY(mt_sync(e));
            e->pregen_lane = v != 0;
        }
    }
    else if (!strcmp(name, "lookahead_streams")) BBAI_TRY(set_sides(e, v));
    else if (!strcmp(name, "gate_fault_inject")) e->host_flags[0] = v != 0;       // tests: what a timed-out gate leaves behind
    else if (k && !k->read_only) {
        if (k->field == &bbai_env::render_piece_bytes && v != 64 && v != 128) ARG_FAIL("render_piece_bytes: 64 or 128");
        if (k->field == &bbai_env::rt_next_ts && v != 8 && v != 16 && v != 32) ARG_FAIL("render_target_tile_size: 8, 16 or 32");
        e->*k->field = knob_value(*k, v);
        if (k->field == &bbai_env::render_delta) invalidate_target(e->targets.view);
        if (k->field == &bbai_env::gate_probe) { e->n_probed = 0; e->gate_forced = 0; }      // (forget the verdicts: the next window probes again)
    }
    else {
        snprintf(g_err, sizeof(g_err), "set_option: unknown option '%s'", name);
        return BBAI_ERR_ARG;
    }
    return BBAI_OK;
}

static int read_flow(bbai_env* e, int word, unsigned long long* out) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, e->flow + word, 8, hipMemcpyDeviceToHost));
    return BBAI_OK;
}

// Read back a knob: every row of KNOBS, plus what is computed on the way out.  ("gate_fault_inject" is write only.)
int bbai_get_option(bbai_env* e, const char* name, int64_t* out) {
    if (!e || !name || !out) ARG_FAIL("null handle, name or output");
    if (const Knob* k = find_knob(name)) *out = e->*k->field;
    else if (!strcmp(name, "render_delta_valid")) *out = e->targets.view.valid ? 1 : 0;
    else if (!strcmp(name, "grid_delta_valid")) *out = e->targets.grid.valid ? 1 : 0;
    else if (!strcmp(name, "gate_fault")) *out = e->host_flags ? (int64_t)e->host_flags[0] : 0;     // sticky; no synchronisation
    else if (!strcmp(name, "profile_step_ticks")) *out = e->prof_step_ticks;
    else if (!strcmp(name, "cplane")) *out = e->cplane ? 1 : 0;
    else if (!strcmp(name, "owned")) *out = (int64_t)e->own.held.size();      // device allocations, the pinned words, streams and events held right now
    else if (!strcmp(name, "gate_timeouts")) {      // (synchronises) window gates that gave up waiting for a refill: must be 0 (k_gate)
        ON_DEVICE(e->device);
        unsigned long long v = 0;
        BBAI_TRY(read_flow(e, FLOW_GATE_TIMEOUTS, &v));
        *out = (int64_t)v;
    }
    else if (!strcmp(name, "render_pace_effective")) *out = e->render_pace > 0 ? e->render_pace : 0;
    else {
        snprintf(g_err, sizeof(g_err), "get_option: unknown option '%s'", name);
        return BBAI_ERR_ARG;
    }
    return BBAI_OK;
}

int bbai_profile(bbai_env* e, int enable) {
    if (!e) ARG_FAIL("null handle");
    e->prof_on = enable != 0;
    // 1: start from zero; 2: resume (totals kept: callers that bracket every other block of a run); 0: pause, totals readable
    if (enable == 1) e->prof_step_ticks = 0;
    if (enable == 1) for (int k = 0; k < 3; ++k) { e->prof_ms[k] = 0; e->prof_n[k] = 0; for (int i = 0; i < PROF_RING; ++i) e->prof[k][i].used = false; }
    return BBAI_OK;
}

int bbai_profile_read(bbai_env* e, double* ms_total /* [3] */, int64_t* launches /* [3] */) {
    if (!e || !ms_total || !launches) ARG_FAIL("null pointer");
    ON_DEVICE(e->device);
    for (int k = 0; k < 3; ++k) {
        for (int i = 0; i < PROF_RING; ++i) prof_fold(e, k, i);
        ms_total[k] = e->prof_ms[k]; launches[k] = e->prof_n[k];
    }
    return BBAI_OK;
}

int bbai_generator_failures(bbai_env* e, uint64_t* out) {
    if (!e || !out) ARG_FAIL("null pointer");
    ON_DEVICE(e->device);
    unsigned long long v = 0;
    BBAI_TRY(read_flow(e, FLOW_GEN_FAILURES, &v));
    *out = (uint64_t)v;
    return BBAI_OK;
}

int bbai_reset_count(bbai_env* e, uint64_t* out) {
    if (!e || !out) ARG_FAIL("null pointer");
    ON_DEVICE(e->device);
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long shards[SHARDS * SHARD_U64], v = 0;
    HIP_TRY(hipMemcpy(shards, e->totals, sizeof(shards), hipMemcpyDeviceToHost));
    for (int k = 0; k < SHARDS; ++k) v += shards[k * SHARD_U64];
    *out = (uint64_t)v;
    return BBAI_OK;
}


// ---- device snapshots (bbai_statek.hpp): the live state of listed envs, out and back in, as launches on the caller's stream ----------------
// (They close this file on purpose: bbai_statek.hpp says why.)  Neither is a consume-tick: the look-ahead ring, the windows' bookkeeping, e->tick, the RNG streams and the gate stay as they are.
static unsigned state_grid(int64_t count) { return (unsigned)std::min<int64_t>((count + 3) / 4, 65536); }        // one wave per list entry

int bbai_save_state(bbai_env* e, const int64_t* ids, int64_t count, uint8_t* rec, uint8_t* hot, uint64_t* stale, uint8_t* lsm, void* stream) {
    if (!e || count < 0) ARG_FAIL("null handle or negative count");
    if (count == 0) return BBAI_OK;
    if (!rec || !hot || !stale) ARG_FAIL("null snapshot buffer");
    if (((uintptr_t)rec | (uintptr_t)hot) & 15) ARG_FAIL("snapshot records and hot states must be 16-byte aligned");
    if (!ids && count > e->n) ARG_FAIL("count > n_envs without ids");
    if (e->cfg.rec_bytes > STATE_MAX_REC || (e->cfg.rec_bytes & 15)) ARG_FAIL("record size not covered by the snapshot kernels");
    if (!e->live) { snprintf(g_err, sizeof(g_err), "save_state before reset"); return BBAI_ERR_STATE; }
    ON_DEVICE(e->device);
    hipStream_t s = (hipStream_t)stream;
    CallScope call(e, s);
    BBAI_TRY(call.rc);
    hipLaunchKernelGGL(k_state_save<0>, dim3(state_grid(count)), dim3(256), 0, s, e->cfg, e->n, ids, count, e->rec, e->inplace ? e->next_rec : nullptr, e->depth,
                       e->hot, e->stale, e->lsm, rec, (u32x4*)hot, stale, lsm);
    HIP_TRY(hipGetLastError());
    return call.leave();
}

int bbai_load_state(bbai_env* e, const int64_t* ids, const int64_t* rows, int64_t count, int64_t snap_rows, const uint8_t* rec, const uint8_t* hot,
                    const uint64_t* stale, const uint8_t* lsm, uint8_t* image, uint8_t* dirs, void* stream) {
    if (!e || count < 0 || snap_rows < 0) ARG_FAIL("null handle or negative count");
    if (count == 0) return BBAI_OK;
    if (!rec || !hot || !stale || !image || !dirs) ARG_FAIL("null snapshot or observation buffer");
    if (((uintptr_t)rec | (uintptr_t)hot) & 15) ARG_FAIL("snapshot records and hot states must be 16-byte aligned");
    if (!ids && count > e->n) ARG_FAIL("count > n_envs without ids");
    if (!rows && count > snap_rows) ARG_FAIL("count > snap_rows without rows");
    if (e->cfg.rec_bytes > STATE_MAX_REC || (e->cfg.rec_bytes & 15)) ARG_FAIL("record size not covered by the snapshot kernels");
    if (!e->seeded) { snprintf(g_err, sizeof(g_err), "load_state before seed"); return BBAI_ERR_STATE; }
    ON_DEVICE(e->device);
    hipStream_t s = (hipStream_t)stream;
    CallScope call(e, s);
    BBAI_TRY(call.rc);
    hipLaunchKernelGGL(k_state_load<0>, dim3(state_grid(count)), dim3(256), 0, s, e->cfg, e->n, ids, rows, count, snap_rows, rec, (const u32x4*)hot, stale, lsm,
                       e->rec, e->inplace ? e->next_rec : nullptr, e->depth, e->hot, e->stale, e->lsm, e->vhead, e->vset, e->vplane, e->cplane, e->fcache,
                       e->bot_state, e->bot_stack, image, dirs);
    if (e->tokens)
        hipLaunchKernelGGL(k_state_tokens<0>, dim3((unsigned)std::min<int64_t>((count + 63) / 64, 4096)), dim3(64), 0, s, e->cfg, e->n, ids, rows, count, snap_rows,
                           e->rec, e->inplace ? e->next_rec : nullptr, e->depth, e->hot, e->tokens);
    HIP_TRY(hipGetLastError());
    e->live = true;
    return call.leave();
}

// ---- env.seed(s); env.reset() for listed envs of a live batch (bbai_reseedk.hpp) ------------------------------------------------------------
// (Behind the snapshots, for the same reason: its kernels' code lies behind every earlier kernel's.)
// Not a consume-tick: e->tick stays, no gate, no refill launch.  What orders it is events alone:
//   1. the first look-ahead stream waits for the caller's stream (the call's ids and seeds; every step enqueued before) and for the other look-ahead
//      streams -- so it stands behind EVERY refill launched so far; there k_reseed_seed and the generation of the listed envs' rings run (an
//      env's MT19937 state keeps one writer at a time: its refills before, this generation, its refills after -- the latter behind ev_consumed of
//      a window_end the caller's stream enqueues after this call);
//   2. the caller's stream waits for the end of that generation, and only then consumes slot 0 of the new rings (k_reseed_consume).
// After step 1 every closed window's refill has landed -- all their `pending` bytes are zero -- so the current window's buffer is the only one that can
// hold a listed env, and k_reseed_seed clears it there.  k_reseed_consume then books the env's reset into that buffer like any finished env's.
// Option "reseed_levels" = k (0 < k < D - inplace): only levels 0 .. k - 1 of the new stream are generated, into slots 0 .. k - 1.  Slot k keeps the
// empty FROZEN hot state that k_reseed_seed wrote into every slot, so the env's ordinary move into it -- at the end of its k-th level under
// auto-reset, or by the bbai_reset behind it -- PARKS the env: frozen, like an env that finished without auto-reset, until it is reseeded or
// the batch is seeded.  Nothing else changes: same kernels, same order, same bookkeeping (the move is counted and booked for the window's
// refill like any other; what the refill puts into the slots behind a parked env is never played).  bbai_reseedk.hpp says why every slot an env
// can park in holds a record that is safe to move into.
static int reseed_scratch(bbai_env* e) {
    if (e->rs_claim) return BBAI_OK;          // (the group is committed as a whole: any of its fields says so)
    const size_t n = (size_t)e->n;
    Scoped call, done, part[MAX_SIDES], list, count, pending, first, claim;
    BBAI_TRY(call.event()); BBAI_TRY(done.event());
    for (int k = 1; k < MAX_SIDES; ++k) BBAI_TRY(part[k].event());
    BBAI_TRY(list.mem((size_t)SHARDS * (size_t)gen_sublist_cap(e->n) * 4)); BBAI_TRY(count.mem(SHARDS * GEN_COUNT_U32 * 4));
    BBAI_TRY(pending.mem(n, true)); BBAI_TRY(first.mem(n, true));
    BBAI_TRY(claim.mem((n + 31) / 32 * 4));
    if (hipMemset(claim.h, 0, (n + 31) / 32 * 4) != hipSuccess) { snprintf(g_err, sizeof(g_err), "reseed: hipMemset failed"); return BBAI_ERR_HIP; }
    Owner& o = e->own;
    for (int k = 1; k < MAX_SIDES; ++k) o.adopt(&e->ev_rs_part[k], part[k]);
    o.adopt(&e->ev_rs_call, call); o.adopt(&e->ev_rs_done, done); o.adopt(&e->rs_list, list); o.adopt(&e->rs_count, count); o.adopt(&e->rs_pending, pending); o.adopt(&e->rs_first, first); o.adopt(&e->rs_claim, claim);
    return BBAI_OK;
}

int bbai_reseed(bbai_env* e, const int64_t* ids, const uint64_t* seeds, int64_t count, uint8_t* image, uint8_t* dirs, void* stream) {
    if (!e || count < 0) ARG_FAIL("null handle or negative count");
    if (!seeds || !image || !dirs) ARG_FAIL("null seed list or observation buffer");
    if (!ids && count > e->n) ARG_FAIL("count > n_envs without ids");
    if (!e->seeded) { snprintf(g_err, sizeof(g_err), "reseed before seed"); return BBAI_ERR_STATE; }
    if (!e->live && !(ids == nullptr && count == e->n)) {
        snprintf(g_err, sizeof(g_err), "reseed of listed envs before reset (a handle that was never reset takes every env: ids = NULL, count = n_envs)");
        return BBAI_ERR_STATE;
    }
    if (count == 0) return BBAI_OK;
    ON_DEVICE(e->device);
    hipStream_t s = (hipStream_t)stream;
    CallScope call(e, s);
    BBAI_TRY(call.rc);
    BBAI_TRY(reseed_scratch(e));
    const TickPos tp = tick_pos(e);           // (at a window's first tick: the window about to open -- its gate, still to come, clears only its meta line)
    uint8_t* const cur_pending = e->pending + (size_t)tp.wb * e->n;
    uint8_t* const cur_first = e->first_slot + (size_t)tp.wb * e->n;
    hipStream_t g = e->side;
    const int full = e->depth - e->inplace;           // levels of a whole ring; a depth of 0, or of that many and more, is the whole ring
    const int gen = e->reseed_levels > 0 && e->reseed_levels < full ? e->reseed_levels : full;
    HIP_TRY(hipEventRecord(e->ev_rs_call, s));
    HIP_TRY(hipStreamWaitEvent(g, e->ev_rs_call, 0));
    for (int k = 1; k < e->n_sides; ++k) {
        HIP_TRY(hipEventRecord(e->ev_rs_part[k], e->sides[k]));
        HIP_TRY(hipStreamWaitEvent(g, e->ev_rs_part[k], 0));
    }
    HIP_TRY(hipMemsetAsync(e->rs_count, 0, SHARDS * GEN_COUNT_U32 * 4, g));
    hipLaunchKernelGGL(k_reseed_seed<0>, dim3((unsigned)std::min<int64_t>((count + 63) / 64, 65536)), dim3(64), 0, g, e->n, ids, seeds, count, e->mt, e->mti, e->mtpar,
                       e->hot, e->next_hot, e->depth, e->depth - gen, cur_pending, e->rs_pending, e->rs_first, e->rs_claim, e->rs_list, e->rs_count);
    launch_pregen(e, pregen_grid(e, count), true, e->rs_pending, e->rs_first, count, 0, e->rs_list, e->rs_count);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e->ev_rs_done, g));
    HIP_TRY(hipStreamWaitEvent(s, e->ev_rs_done, 0));
    hipLaunchKernelGGL(k_reseed_consume<0>, dim3(state_grid(count)), dim3(256), 0, s, e->cfg, e->n, ids, count, e->rs_claim, e->rec, e->hot, e->stale, e->next_rec, e->next_hot,
                       e->vhead, e->vset, e->totals, e->depth, cur_pending, cur_first, e->win_meta + (size_t)tp.wb * META_U32, image, dirs, e->vplane, e->fcache, e->lsm,
                       e->inplace, e->cplane, e->bot_state, e->bot_stack);
    if (e->tokens)
        hipLaunchKernelGGL(k_state_tokens<0>, dim3((unsigned)std::min<int64_t>((count + 63) / 64, 4096)), dim3(64), 0, s, e->cfg, e->n, ids, (const int64_t*)nullptr, count, count,
                           e->rec, e->inplace ? e->next_rec : nullptr, e->depth, e->hot, e->tokens);
    HIP_TRY(hipGetLastError());
    e->live = true;
    return call.leave();
}

// bbai_import_state's token rows: the registered rows of envs [first, first + count) from their live records, by k_state_tokens over a device id
// list of the range.  Synchronous, like the import; it stands here and not next to its caller so that k_state_tokens' first launch stays
// bbai_load_state's (bbai_statek.hpp: a template's code is emitted where it is first launched).
static int import_tokens(bbai_env* e, int64_t first, int64_t count) {
    std::vector<int64_t> ids((size_t)count);
    for (int64_t k = 0; k < count; ++k) ids[(size_t)k] = first + k;
    Scoped list;
    BBAI_TRY(list.mem((size_t)count * sizeof(int64_t)));
    HIP_TRY(hipMemcpy(list.h, ids.data(), (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_state_tokens<0>, dim3((unsigned)std::min<int64_t>((count + 63) / 64, 4096)), dim3(64), 0, 0, e->cfg, e->n, (const int64_t*)list.h,
                       (const int64_t*)nullptr, count, count, e->rec, e->inplace ? e->next_rec : nullptr, e->depth, e->hot, e->tokens);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return BBAI_OK;
}

}  // extern "C"
