/* bbai.h -- C ABI of the MI355X batched BabyAI environment engine (libbbai_hip.so).
 *
 * The reference (mila-iqia/babyai) is pure Python and has no FFI; this ABI is the
 * native boundary UNDER the Python adapter that mirrors the reference's env protocol.
 * Each entry point names the reference interface it replaces (file:line under
 * /root/reference).  All device pointers are caller-owned HBM buffers (e.g. the
 * data_ptr() of torch tensors on the handle's device); launches are asynchronous on
 * the caller's hipStream_t (passed as void*; NULL = default stream).  No exceptions
 * cross the boundary: every call returns 0 or a negative bbai_status.  One handle per
 * device; a handle is not thread-safe and follows ONE caller stream at a time: a call that arrives on a different
 * stream than the previous one is ordered (by an event) behind everything the handle enqueued before.  By default that
 * event is recorded on the previous stream at the moment of the switch, so the previous stream must still exist then;
 * see bbai_set_call_events for callers that create and destroy streams.
 */
#ifndef BBAI_H
#define BBAI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum bbai_status {
    BBAI_OK = 0,
    BBAI_ERR_ARG = -1,        /* bad argument / unsupported level configuration */
    BBAI_ERR_HIP = -2,        /* HIP runtime error (see bbai_last_error) */
    BBAI_ERR_STATE = -3,      /* call order violated (e.g. step before seed+reset) */
    BBAI_ERR_NOMEM = -4
};

/* Level description: the constructor arguments of a reference level class
 * (babyai/levels/iclr19_levels.py; LevelGen babyai/levels/levelgen.py:262-291) as data.
 * Layout fields (W..rec_bytes) are derived by bbai_fill_layout. */
typedef struct bbai_level_cfg {
    int32_t kind;                       /* 0 = GoTo family, 1 = LevelGen family, 2 = bonus-level scripts */
    int32_t room_size, num_rows, num_cols, num_dists;
    int32_t redball, connect, check_reach, doors_open, all_unique;     /* GoTo family */
    int32_t instr, target, lock, lock_color_excl, dists_per_room, grey_dists;   /* single-instruction levels */
    int32_t script, sp[4];              /* kind 2: bonus_levels.py gen_mission script id + parameters */
    int32_t locations, unblocking, implicit_unlock;                    /* LevelGen */
    int32_t n_action_kinds, action_kinds[4];    /* 0 goto 1 pickup 2 open 3 putnext, in list order */
    int32_t n_instr_kinds, instr_kinds[3];      /* 0 action 1 and 2 seq, in list order */
    double locked_room_prob;
    int32_t W, H, ES, EH, maxo;
    int32_t off_I, off_app, off_pos, off_cont, off_prog, rec_bytes;
} bbai_level_cfg;

typedef struct bbai_env bbai_env;       /* opaque: N envs of one level on one device */

#define BBAI_OBS_BYTES 147              /* uint8[7][7][3], image[view_x][view_y][channel] */
#define BBAI_PIX_BYTES 9408             /* uint8[56][56][3], RGBImgPartialObsWrapper, tile 8 */
#define BBAI_PROG_BYTES 112             /* compiled instruction tree (mission descriptor) */
#define BBAI_TILE_BYTES 192

int bbai_version(void);
const char* bbai_last_error(void);

/* Derive the record layout for a level configuration. */
int bbai_fill_layout(bbai_level_cfg* cfg);

/* gym.make(id) x n_envs (babyai/levels/levelgen.py:467-493 registration; scripts/train_rl.py:53-60
 * builds the env list).  Allocates all per-env state in HBM on `device`.
 * State layout (an internal choice, never visible in results; bbai_get_option "inplace" reports it, BBAI_INPLACE=1 / 0 forces it): every
 * env owns a ring of pre-generated levels (its RNG stream, generated ahead of need).  Classic: a live record per env, a finished env's
 * next level is copied out of its ring slot.  In-place: the live record IS the ring slot the episode was generated into and a
 * finished env just moves on to the next slot -- no copy and no second launch behind a step; chosen for single-room levels while the
 * ring stays under 12 GiB (the reset-heavy single-room batches: 2 % of the envs finish on every step there), see DESIGN.md section 5. */
int bbai_create(const bbai_level_cfg* cfg, int64_t n_envs, int device, bbai_env** out);
void bbai_destroy(bbai_env* env);

/* env.seed(s) for every env (scripts/train_rl.py:59, babyai/evaluate.py:67-68,105-106):
 * seeds_host[i] (8 bytes per env cross PCIe) -> gym-style sha512 -> MT19937 init_by_array, per lane on the device;
 * then the first levels of every env's stream are generated ahead of need.  Synchronous. */
int bbai_seed(bbai_env* env, const uint64_t* seeds_host, int64_t n);

/* env.reset() for every env (babyai/levels/levelgen.py:35-47; ParallelEnv.reset
 * babyai/rl/utils/penv.py:39-43; ManyEnvs.reset babyai/evaluate.py:68-71): generates the next
 * level of each env's RNG stream on the device and writes the first observation. */
int bbai_reset(bbai_env* env, uint8_t* image_dev, uint8_t* dir_dev, void* stream);

/* env.step(action) for every env (babyai/levels/levelgen.py:49-66).
 *   auto_reset != 0 : ParallelEnv semantics (babyai/rl/utils/penv.py:8-11,45-52): a finished env
 *                     is reset in the same call and image/dir hold the NEXT episode's first obs,
 *                     while reward/done are the terminal step's.
 *   auto_reset == 0 : ManyEnvs semantics (babyai/evaluate.py:73-81): a finished env is frozen and
 *                     keeps re-emitting its last (obs, reward, done) until bbai_reset.
 * actions_dev[i] is 0..6 (MiniGridEnv.Actions), or BBAI_ACTION_RESET_ENV = "env.reset() for this env now": the
 * episode is abandoned with done = 1, reward = 0 and handled like any finished env above (a ParallelEnv worker's
 * `reset` command, penv.py:12-14; scripts/make_agent_demos.py:84-88 after a bot crash).
 * UNKNOWN ACTIONS: the reference asserts on an action outside its enum (gym_minigrid MiniGridEnv.step: `assert False,
 * "unknown action"`, reached from levelgen.py:50).  A kernel cannot raise: bytes 8..255 are DEFINED here as the `done`
 * action (no movement; the step is counted, the verifier sees a done action).  Callers that want the reference's
 * behaviour check their actions first: the Python binding does (BatchedBabyAIEnv(validate_actions=True) / step(...,
 * validate=True): one device-side max-reduce and a host sync, off by default; the list-of-dicts adapters, whose actions
 * are host arrays anyway, always check and raise AssertionError("unknown action")).
 * reward_dev[i]   = float32 rounding of the reward (what babyai/rl/algos/base.py:162-167 makes of it);
 * reward64_dev[i] = the reference's own return value: MiniGridEnv._reward() as a Python float (levelgen.py:59-61),
 *                   bit for bit (what babyai/evaluate.py:128 accumulates).  May be NULL.
 * THE HOLD ACTION: under bbai_set_option(env, "step_hold", 1) an env whose byte is BBAI_ACTION_HOLD takes no part in the step -- the way to
 * step only some envs of a batch (expand a stored state, evaluate a few, step the envs whose actions are ready).  Its state, step_count,
 * level stream, lastStepMatch byte and the expert's view of it are untouched; its rows of image_dev / dir_dev are written again unchanged;
 * its entries of reward_dev / reward64_dev / done_dev are LEFT ALONE -- the frozen env's contract: the caller's buffers must hold the env's
 * last outputs.  A frozen or parked env that holds stays frozen or parked; BBAI_ACTION_RESET_ENV is unaffected.  A 64-env block (envs
 * 64 b .. 64 b + 63) in which every env holds costs one 64-byte load, so a step that holds nearly everybody costs little more than its launch.
 * Honoured by bbai_step, bbai_step_render, bbai_step_full, bbai_step_tapped (a held listed env logs its unchanged outputs) and, per tick,
 * bbai_rollout; never by bbai_bot_rollout (its actions are the expert's).  With the option at 0 (default) byte 8 is `done` like 9..255. */
#define BBAI_ACTION_RESET_ENV 7
#define BBAI_ACTION_HOLD 8
int bbai_step(bbai_env* env, const uint8_t* actions_dev, uint8_t* image_dev, uint8_t* dir_dev,
              float* reward_dev, double* reward64_dev, uint8_t* done_dev, int auto_reset, void* stream);

/* RGBImgPartialObsWrapper.observation (gym_minigrid.wrappers; used at babyai/evaluate.py:91-92,
 * scripts/train_rl.py:57-58): encoded obs uint8[N][147] -> pixels uint8[N][56][56][3].
 * The tile atlas must have been installed with bbai_set_atlas. */
int bbai_set_atlas(bbai_env* env, const uint8_t* tiles_host, int n_tiles, const uint8_t* lut_host /* [2][256] */);
int bbai_render(bbai_env* env, const uint8_t* image_dev, uint8_t* pixels_dev, void* stream);

/* env.step(action) of a batch wrapped in RGBImgPartialObsWrapper (babyai/evaluate.py:91-92: `env = RGBImgPartialObsWrapper(env)`, whose
 * step() returns the rendered observation) as ONE call: exactly bbai_step followed by bbai_render(image_dev -> pixels_dev), same bytes.
 * With option "step_render_split" = 1 (and a batch of 262 144 envs or more, auto-reset consumed inside the step kernel) the batch is stepped
 * in two halves and the second half's step kernel runs on a stream of the handle's own UNDER the first half's render; everything is joined
 * on `stream` before the call's last launch, so callers see no difference but the time. */
int bbai_step_render(bbai_env* env, const uint8_t* actions_dev, uint8_t* image_dev, uint8_t* dir_dev, float* reward_dev,
                     double* reward64_dev, uint8_t* done_dev, int auto_reset, uint8_t* pixels_dev, void* stream);

/* Delta rendering.  bbai_set_render_target registers a caller-owned uint8[N][56][56][3] pixel buffer (NULL unregisters) and says:
 * "only this handle's renders write here".  The handle then keeps the atlas tile id of every cell of the frame the buffer holds
 * (49 bytes per env, allocated at the first registration), and a render into the buffer -- bbai_render, bbai_step_render (split
 * or not), bbai_rollout with pixels -- stores only the 128-byte lines whose cells changed since the frame before: same bytes, a
 * fraction of the stores (how large a fraction depends on the actions: turns redraw most of the view, blocked moves and object
 * actions almost nothing).  The first render after registration, after bbai_set_atlas, after bbai_render_invalidate, after
 * option "render_delta" was set and after a failed launch writes every byte.  Renders into any other buffer are full renders and leave the history alone;
 * a full render into the registered buffer by another path (render_delta 0, a buffer not 128-byte aligned) invalidates it.
 * A caller that writes into the registered buffer itself calls bbai_render_invalidate before the next render.  Register the
 * buffer again when it is reallocated: a freed buffer's address may be handed out again with other contents.
 * Option "render_target_tile_size" (8 by default; 16 or 32) states the frame size of the NEXT registration: uint8[N][7 ts][7 ts][3].  A
 * handle has one target at a time; registering replaces it and invalidates the history.  A target of 16 / 32 is bbai_render_view's (below):
 * the tile ids are those of that size's view atlas, bbai_set_view_atlas of that size invalidates (bbai_set_atlas does not), and
 * bbai_render, bbai_step_render and bbai_rollout treat the handle as one without a target -- but for the one rule below.
 * bbai_render_shadow, bbai_render_invalidate and the options "render_delta" / "render_delta_valid" work alike at every size.
 * What drops the history -- one list, for this target and for the full-grid target (bbai_grid_target.h) alike: a registration; the
 * target's atlas of the registered tile size installed again; its invalidate entry; a set of "render_delta" (this target only); a
 * render that failed; and EVERY entry of this handle that writes frames or observations into a buffer whose bytes overlap the
 * registered ones without being a planned render of that target's envs into their own rows -- bbai_render, bbai_step_render,
 * bbai_rollout's pixels, bbai_render_view, bbai_render_view_pixels, bbai_render_grid, bbai_observe_full, bbai_observe_view, the `full` /
 * `view` frames of bbai_step_full / bbai_step_view, and a render into the other target where the two buffers overlap.  A write that
 * overlaps neither buffer changes nothing.  (The encoded `image`, `dir` and reward outputs of the step entries, rollout and tap rows and
 * the demo entries are not frames and are not looked at: do not point them into a registered buffer.) */
int bbai_set_render_target(bbai_env* env, uint8_t* pixels_dev);
int bbai_render_invalidate(bbai_env* env);
/* A copy of the registered buffer's tile ids, uint8[N][49] (cell = 7 x + y of the encoded view), into a device buffer, on `stream`:
 * what the next delta render compares against (tests). */
int bbai_render_shadow(bbai_env* env, uint8_t* out_dev, void* stream);

/* The full-grid picture: MiniGridEnv.render('rgb_array', highlight, tile_size) (gym_minigrid minigrid.py; called by
 * scripts/manual_control.py:14 with --tile_size, scripts/enjoy.py:101,108 in 'human' mode) of listed envs, on the device.
 * bbai_set_grid_atlas installs the tile atlas of one tile size (8, 16 or 32; babyai_amd/data/grid_atlas_ts<size>.npz, made by
 * tools/gen_grid_atlas.py): tiles uint8[n_tiles][ts][ts][3], n_tiles <= 132, and lut[highlight][agent][key] (agent = 0, or 1 + the
 * agent's direction on that cell; key = type | colour << 3 | state << 6); synchronous.  A handle keeps the atlas of every tile size
 * installed on it.  BBAI_ERR_ARG for another tile size, a tile count out of range or a lut entry >= n_tiles.
 * bbai_render_grid writes frame k = the picture of env ids_dev[k] (int64 device array; NULL = envs 0 .. count - 1) into
 * out_dev + k * H*ts * W*ts * 3 (16-byte aligned), pixel [row y][column x][rgb] as Grid.render lays it out: the grid's cells, the
 * agent's triangle on its cell, and -- highlight != 0 -- the cells the agent sees lightened (the carried object is not drawn).  It
 * reads the current state and writes nothing but out_dev (no state; where out_dev overlaps a registered target: the list above);
 * asynchronous on `stream`, ordered behind the handle's previous calls like every state-reading call.  An id outside [0, n) yields an
 * all-zero frame, never an out-of-bounds read.  BBAI_ERR_STATE without an atlas of that tile size or before the first reset;
 * BBAI_ERR_ARG for a tile size other than 8 / 16 / 32, count < 0, count > n without ids, or a missing / misaligned out_dev. */
int bbai_set_grid_atlas(bbai_env* env, int tile_size, const uint8_t* tiles_host, int n_tiles,
                        const uint8_t* lut_host /* [2][5][256] */);
int bbai_render_grid(bbai_env* env, int tile_size, int highlight, const int64_t* ids_dev /* NULL = envs 0..count-1 */,
                     int64_t count, uint8_t* out_dev /* [count][H*ts][W*ts][3] */, void* stream);

/* The agent's 7x7 view as pixels at tile sizes 16 and 32: RGBImgPartialObsWrapper(env, tile_size).observation (gym_minigrid
 * wrappers.py; scripts/manual_control.py --agent_view, and 7 x 32 = 224 / 7 x 16 = 112 pixel inputs of image models).  Tile size 8 is
 * bbai_set_atlas / bbai_render (and its delta render); the delta render at these sizes is the last paragraph.
 * bbai_set_view_atlas installs the tile atlas of one tile size (babyai_amd/data/tile_atlas_ts<size>.npz, made by tools/gen_atlas.py
 * --tile-size): tiles uint8[n_tiles][ts][ts][3], n_tiles <= 64, and lut[agent cell][key] as bbai_set_atlas takes it (row 0 = ordinary
 * view cell, row 1 = the agent's cell (3, 6); key = type | colour << 3 | state << 6, taken & 255); synchronous.  A handle keeps the atlas
 * of each size installed on it.  BBAI_ERR_ARG for a tile size other than 16 / 32, a tile count out of range or a lut entry >= n_tiles.
 * bbai_render_view reads rows of an ENCODED observation buffer image_dev uint8[rows][147] (indexed [x][y][3]: the caller's buffer, not
 * engine state -- the current observations or stored ones) and writes frame k = the picture of row ids_dev[k] (int64 device array;
 * NULL = rows 0 .. count - 1) into out_dev + k * 147 * ts * ts (16-byte aligned): uint8[7 ts][7 ts][3], pixel [row = view y][column =
 * view x][rgb] -- 37 632 bytes a frame at 16, 150 528 at 32.  It writes nothing but out_dev; asynchronous on `stream`, ordered like
 * every other call of the handle.  An id outside [0, rows) yields an all-zero frame, never an out-of-bounds read.  BBAI_ERR_STATE
 * without an atlas of that tile size; BBAI_ERR_ARG for a tile size other than 16 / 32, count < 0, count > rows without ids, or a
 * missing / misaligned out_dev.
 * Delta render: a call that draws the WHOLE batch into the target registered at this tile size (bbai_set_render_target under option
 * "render_target_tile_size": out_dev = the registered pointer, 64-byte aligned, ids_dev = NULL, count = rows = n_envs, option
 * "render_delta" not 0) stores only the 64-byte pieces of each frame that show a cell whose atlas tile changed since the frame the buffer
 * holds, and brings the tile ids up to date -- the same bytes in the buffer as a whole render's, a fraction of the stores.  The first such
 * call after a registration, bbai_set_view_atlas of this size, bbai_render_invalidate, a set of "render_delta" or a failed launch draws the
 * frames whole and writes every tile id.  Every other bbai_render_view whose output range overlaps the registered buffer (ids given, a
 * partial count, another tile size, a misaligned target, "render_delta" 0) draws whole frames and invalidates the history; one that
 * writes elsewhere leaves it alone. */
int bbai_set_view_atlas(bbai_env* env, int tile_size, const uint8_t* tiles_host, int n_tiles, const uint8_t* lut_host /* [2][256] */);
int bbai_render_view(bbai_env* env, int tile_size, const uint8_t* image_dev /* [rows][147] */, int64_t rows,
                     const int64_t* ids_dev /* NULL = rows 0..count-1 */, int64_t count, uint8_t* out_dev /* [count][7*ts][7*ts][3] */,
                     void* stream);

/* The fully observable encoding: FullyObsWrapper.observation (gym_minigrid wrappers.py; restated in
 * oracle/shim/gym_minigrid/wrappers.py:39-56) -- grid.encode() of the whole W x H grid, indexed [x][y], cell = (type, colour,
 * state), the agent's cell overwritten with (10 = agent, 0 = red, agent_dir) -- on the device.
 * bbai_observe_full (replaces FullyObsWrapper(env).observation(obs)['image'] of the current state) writes frame k = env ids_dev[k]
 * (int64 device array; NULL = envs 0 .. count - 1) into out_dev + k * W*H*3 (16-byte aligned).  It reads the current state and writes
 * nothing but out_dev; asynchronous on `stream`, ordered behind the handle's previous calls.  An id outside [0, n) yields an all-zero
 * frame.  BBAI_ERR_STATE before the first reset; BBAI_ERR_ARG for count < 0, count > n without ids, or a missing / misaligned out_dev.
 * bbai_step_full (replaces FullyObsWrapper(env).step for every env): bbai_step, then the full observation of EVERY env of the state the
 * step leaves behind -- a finished env's next episode under auto_reset, a frozen env's final state without -- into
 * full_dev[n][W][H][3] (16-byte aligned), as ONE call.  image_dev (the 7x7 view) is written as by bbai_step. */
int bbai_observe_full(bbai_env* env, const int64_t* ids_dev /* NULL = envs 0..count-1 */, int64_t count,
                      uint8_t* out_dev /* [count][W][H][3] */, void* stream);
int bbai_step_full(bbai_env* env, const uint8_t* actions_dev, uint8_t* image_dev, uint8_t* dir_dev, float* reward_dev,
                   double* reward64_dev, uint8_t* done_dev, int auto_reset, uint8_t* full_dev /* [n][W][H][3] */, void* stream);

/* Mission text as token ids, device-resident (replaces the per-step regex tokenisation of every mission in
 * InstructionsPreprocessor, babyai/utils/format.py:59-75): register a caller-owned uint8[N][72] buffer; the engine
 * rewrites env i's row whenever env i starts a new episode.  Ids follow babyai_amd/missions.py VOCAB, 0 = padding. */
#define BBAI_TOK_MAX 72
int bbai_set_token_buffer(bbai_env* env, uint8_t* tokens_dev);

/* State access (host buffers; synchronous): parity tests, checkpoints, mission strings.  hot_host[15] is the env's place in its
 * look-ahead ring: engine bookkeeping of the EXPORTING handle -- bbai_import_state ignores it and keeps the importing handle's own
 * (the ring belongs to the handle; in the in-place layout the slot says where the live record is).
 * All three take the env range [first, first + count): BBAI_ERR_ARG for a negative first or count or first + count > n_envs; count == 0
 * is a no-op.  bbai_import_state with records (rec_host != NULL) puts the range's envs into the given states like bbai_load_state: where
 * the expert's state is allocated each env's next bbai_bot_act starts a fresh Bot, a registered token buffer gets the imported missions'
 * tokens in the range's rows, and the lastStepMatch bytes are cleared (they are no part of the exported state); every env keeps its own
 * look-ahead ring and RNG stream, so it goes on with its OWN next level when the imported episode ends.  Unlike bbai_load_state it writes
 * NO observation: the caller's image / direction buffers (and a render target) are stale until the next step or an explicit observe.
 * A hot- or stale-only import (rec_host == NULL: poses of the records the envs hold) changes neither the expert's plans nor token rows. */
int bbai_export_state(bbai_env* env, int64_t first, int64_t count, uint8_t* rec_host,
                      uint8_t* hot_host /* 16 B each */, uint64_t* stale_host);
int bbai_import_state(bbai_env* env, int64_t first, int64_t count, const uint8_t* rec_host,
                      const uint8_t* hot_host, const uint64_t* stale_host);
int bbai_get_programs(bbai_env* env, int64_t first, int64_t count, uint8_t* prog_host /* 112 B each */);

/* Device snapshots: the live state of LISTED envs out of a handle and back into one, as one launch on `stream` -- no host trip, no
 * synchronisation, no allocation; ordered like every other call of the handle.  For level replay (keep a level's first state, replay it
 * later in whichever env is free), look-ahead (one state into seven envs, one action each), backplay and returns to stored states.
 * A snapshot of R rows is four caller-owned device arrays: rec uint8[R][rec_bytes] and hot uint8[R][16] (both 16-byte aligned), stale
 * uint64[R] -- row for row the bytes bbai_export_state returns for that env -- and lsm uint8[R], the env's lastStepMatch byte in the
 * done-action verifier mode (0 otherwise), which is what makes a rewind exact in that mode (bbai_import_state clears it).  It holds an
 * env's LIVE state only: not its look-ahead ring, not its RNG stream, not the expert's plan.  A snapshot is valid in any handle of the
 * same level, rec_bytes and done-action mode, whatever its batch size, state layout or ring depth.
 * bbai_save_state writes row k from env ids_dev[k] (NULL: env k).
 * bbai_load_state loads row rows_dev[k] (NULL: row k) into env ids_dev[k] (NULL: env k): record, hot state (the env keeps its own place
 * in its look-ahead ring: hot[15] of the row is ignored), stale set, lastStepMatch; rebuilds what the handle derives from the record
 * (verifier view, window plane / C plane row, front-cell cache); and writes the env's observation -- gen_obs() of the loaded state -- into
 * row ids_dev[k] of image_dev uint8[n][147] and dir_dev uint8[n].  It writes no other env's bytes and is no consume-tick: the ring, the
 * windows' bookkeeping and the RNG streams are untouched, so when the loaded episode ends the env goes on with its OWN next level.
 * (A snapshot taken right after bbai_reset on a PutNext*Carrying level holds the state AFTER the object was handed to the agent: its
 * gen_obs() differs from the observation bbai_reset returned in that object's cell and the agent's.)  Where the expert's state is
 * allocated the env's next bbai_bot_act starts a fresh Bot.  A registered token buffer gets the loaded missions' tokens in the listed
 * envs' rows.  The registered render target is NOT touched: a caller with one renders afterwards (bbai_render), as after bbai_reset.
 * An id outside [0, n_envs) or a row outside [0, snap_rows) skips that entry; the same row may go to many envs; the same env listed
 * twice gets one of its rows, which one is undefined.  count == 0 is a no-op; BBAI_ERR_ARG for a null handle, a null or misaligned
 * required buffer or a negative count. */
int bbai_save_state(bbai_env* env, const int64_t* ids_dev /* NULL = envs 0..count-1 */, int64_t count, uint8_t* rec_dev, uint8_t* hot_dev,
                    uint64_t* stale_dev, uint8_t* lsm_dev /* may be NULL */, void* stream);
int bbai_load_state(bbai_env* env, const int64_t* ids_dev /* NULL = envs 0..count-1 */, const int64_t* rows_dev /* NULL = row k */, int64_t count,
                    int64_t snap_rows, const uint8_t* rec_dev, const uint8_t* hot_dev, const uint64_t* stale_dev,
                    const uint8_t* lsm_dev /* NULL = zeros */, uint8_t* image_dev, uint8_t* dir_dev, void* stream);

/* env.seed(s); env.reset() for LISTED envs of a live batch, on `stream`, with no host synchronisation, allocation or host copy (the scratch
 * memory of a handle's first call aside).  In the reference a seed belongs to an EPISODE: ManyEnvs.seed(seeds); reset() before every
 * evaluation round (babyai/evaluate.py:64-71,105-106), env.seed(seed + len(demos)) before every demonstration
 * (scripts/make_agent_demos.py:93), env.seed(args.seed + episode_num) (scripts/enjoy.py:123), and per episode in
 * scripts/train_intelligent_expert.py:115.  bbai_seed serves a whole batch from the host; this call serves entry k as
 * env[ids_dev[k]].seed(seeds_dev[k]); env[ids_dev[k]].reset():
 * the env's MT19937 stream restarts from the seed (the sha512 + init_by_array of bbai_seed), LevelGen.locked_room restarts at None, the env's
 * whole look-ahead ring is regenerated from the new stream, the env is put into level 0 of it -- a frozen env is live again -- and that
 * level's first observation is written to row ids_dev[k] of image_dev uint8[n][147] and dir_dev uint8[n].  Per listed env: the stale set
 * and the lastStepMatch byte are cleared, the next bbai_bot_act starts a fresh Bot where the expert's state is allocated, a registered
 * token buffer gets the new mission's row, and bbai_reset_count grows by one.  Every other env goes on exactly as if nothing had happened.
 * It is no consume-tick; the registered render target is NOT touched (render afterwards, as after bbai_reset).  The call's latency is that of
 * ONE env's ring generated in sequence (ring depth x one level), however few envs are listed.
 * A SHORT reseed -- bbai_set_option(env, "reseed_levels", k) with 0 < k < the ring's depth (2 x "lookahead_period") in front of the call --
 * says "this env will play k levels of the seed's stream": only levels 0 .. k - 1 are generated (k levels of latency instead of the ring's),
 * and when the env's k-th level ends under auto_reset the env PARKS: it is frozen like an env that finished without auto-reset -- done stays
 * 1, the reward stays the last episode's, bbai_bot_act / bbai_bot_rollout answer `done` (6) with gave_up = 0 -- under every step entry until it
 * is reseeded (at any depth) or the batch is seeded by bbai_seed.  Without auto_reset the env freezes at the end of each level as ever and
 * the bbai_reset that moves it past its k levels parks it.  bbai_reset_count counts the parking move like any reset.  A parked env's image,
 * direction, mission and token row are unspecified, and so is what its stream would have produced beyond level k - 1: a parked env is
 * reseeded, not reset.  "done stays 1" is said of the buffers the steps write: a step leaves a frozen env's reward and done alone, so in
 * bbai_bot_rollout's HISTORY, where every step has rows of its own, a parked env's reward / done rows are not written at all -- read an env's
 * FIRST done row of a call, as bbai_demo_jobs does.  The window refills regenerate the slots a parked env has left like any others: levels
 * nobody plays, at most k + 1 per parked env.  k = 0 (the default) or k >= the ring's depth is the whole ring, byte for byte as without
 * the option.
 * An id outside [0, n_envs) skips the entry (pad a fixed-length list with -1); the same env listed twice is a caller error (it gets one of
 * its seeds).  BBAI_ERR_ARG, before any device work, for a null handle, null seeds, null outputs, a negative count or count > n_envs without
 * ids; BBAI_ERR_STATE for a handle that was never seeded, and for one that was seeded but not yet reset unless every env is listed (ids_dev =
 * NULL, count = n_envs).  count == 0 is a no-op. */
int bbai_reseed(bbai_env* env, const int64_t* ids_dev /* NULL = envs 0..count-1 */, const uint64_t* seeds_dev /* [count] */,
                int64_t count, uint8_t* image_dev, uint8_t* dir_dev, void* stream);

/* Checkpoint / resume of a whole batch (the reference checkpoints only its model, babyai/utils/model.py:29-32; an
 * auto-resetting env batch additionally needs its RNG streams): the blob holds the live state, every env's MT19937
 * stream, the look-ahead ring with its window bookkeeping, the counters and -- when bbai_bot_act has been used -- the
 * expert's plans.  Loading it into a fresh handle of the same level and batch size continues the run
 * bit-identically, auto-resets included (tests/test_gpu_parity.py::test_checkpoint_resume_*); a handle whose look-ahead
 * period differs (it is chosen from the free memory at bbai_create unless BBAI_LOOKAHEAD pins it) takes the blob's ring shape; a blob of the
 * other state layout (bbai_create), of the other done-action mode, of another expert stack capacity, of another format version or of the
 * wrong size is refused BEFORE the handle is touched: a refused load leaves the handle exactly as it was.  Synchronous, host buffers.
 * Caller-owned buffers are not part of the blob: keep the last observation next to it if it is needed before the next
 * step, and register the token buffer again after a load (bbai_set_token_buffer refills every row of a live handle). */
int64_t bbai_checkpoint_bytes(bbai_env* env);
int bbai_checkpoint_save(bbai_env* env, void* host_buf, int64_t bytes);
int bbai_checkpoint_load(bbai_env* env, const void* host_buf, int64_t bytes);

/* The reference's GOFAI expert for every env: one `Bot.replan(action_taken)` decision each
 * (babyai/bot.py:547-597; callers babyai/utils/agent.py:139-146 BotAgent.act, scripts/make_agent_demos.py:93-107).
 * `prev_actions_dev` = the action each env was actually stepped with since the previous call (advising mode,
 * bot.py:88-98), or NULL = "the suggestion was taken" (replan(None)).  An env whose episode has just started
 * (step_count == 0), or whose expert was not consulted on the previous step, gets a fresh Bot (= `Bot(env)` there) -- so does an env that
 * held since (BBAI_ACTION_HOLD: its step_count did not advance, which to the expert is a step it was not consulted on).  `actions_dev[i]` = suggested action 0..6, or 255 where the reference bot would
 * have raised (assertion / DisappearedBoxError / endless replanning); it stays 255 until the episode ends.
 * Decision-for-decision parity with the reference bot: tests/test_hostsim_bot.py, tests/golden/bot/.
 * The expert's plan lives in the handle (allocated on first use, ~1.7 KB per env) and is not part of
 * bbai_export_state / bbai_import_state: an env that gets a record through bbai_import_state, bbai_load_state or bbai_reseed starts a
 * fresh Bot at its next decision, wherever in its episode the state is. */
int bbai_bot_act(bbai_env* env, const uint8_t* prev_actions_dev, uint8_t* actions_dev, void* stream);
/* The inner loop of expert-driven demonstration generation (scripts/make_agent_demos.py:71-137 generate_demos with
 * BotAgent, babyai/utils/agent.py:139-155) for every env, T steps per call with NO host round trip between the steps:
 *   for t in 0..T-1:  images_out[t], dirs_out[t] (, tokens_out[t]) = the observation (and mission tokens) the expert decides on;
 *                     actions_out[t] = Bot.replan(None) -- a bot that gave up emits BBAI_ACTION_RESET_ENV ("env.reset() on the
 *                     same stream", make_agent_demos.py:84-88) and gave_up_out[t] = 1 there;
 *                     step with ParallelEnv semantics (auto-reset); rewards_out[t], dones_out[t].
 * image_dev / dir_dev hold the CURRENT observation on entry (what the last reset / step / rollout wrote) and on return.
 * History buffers are [T][n_envs] rows of the per-step layouts (147 / 1 / 72 / 1 / 4 / 1 / 1 bytes per env).  tokens_out may
 * be NULL; otherwise a token buffer must be registered (bbai_set_token_buffer).  The expert and the step are the kernels of
 * bbai_bot_act / bbai_step: same decisions, same bytes (tests/test_gpu_parity.py::test_bot_rollout_*). */
int bbai_bot_rollout(bbai_env* env, int T, uint8_t* image_dev, uint8_t* dir_dev, uint8_t* images_out, uint8_t* dirs_out,
                     uint8_t* tokens_out, uint8_t* actions_out, float* rewards_out, uint8_t* dones_out, uint8_t* gave_up_out,
                     void* stream);
/* Bots that gave up so far: by the reference's own rules / because a fixed-size structure of this port overflowed
 * (subgoal stack, 48 entries unless the environment variable BBAI_BOT_STACK says otherwise when the expert is first
 * used; same-colour keys 12).  The reference's stack is an unbounded list: a bot that replans for ever inside one
 * decision, or loops without progress across steps until max_steps, overflows here instead (observed: UnlockToUnlock,
 * 1 in 1024 MiniBossLevel missions); those episodes fail in the reference too. */
int bbai_bot_stats(bbai_env* env, uint64_t* gave_up, uint64_t* capacity);

/* Measurement aid: copy the outputs of the first `count` envs of a batch (image 147 B, direction, float64 reward, done) and
 * the pixel images of the first `pix_count` into caller-owned log rows with ONE launch on `stream` -- the in-run parity tap of
 * bench.py ("first 1024 envs of every shard, every step, all outputs").  pixels / pixels_out may be NULL when
 * pix_count is 0; both must be 16-byte aligned otherwise.  bbai_tap and bbai_gae take no handle: like any HIP call
 * without one they launch on the calling thread's CURRENT device, which must own `stream` and every pointer. */
int bbai_tap(int64_t count, int64_t pix_count, const uint8_t* image_dev, const uint8_t* dir_dev, const double* reward64_dev,
             const uint8_t* done_dev, const uint8_t* pixels_dev, uint8_t* image_out, uint8_t* dir_out, double* reward64_out,
             uint8_t* done_out, uint8_t* pixels_out, void* stream);
/* The same for an arbitrary list of envs: ids_dev int64[count] on the device, env ids_dev[k] -> log row k (pixels of the
 * first pix_count <= count listed envs).  bench.py taps ids scattered over the whole shard (both ends, block and wave
 * boundaries, a pseudo-random spread: babyai_amd/shard.py scattered_ids). */
int bbai_tap_ids(int64_t count, int64_t pix_count, const int64_t* ids_dev, const uint8_t* image_dev, const uint8_t* dir_dev,
                 const double* reward64_dev, const uint8_t* done_dev, const uint8_t* pixels_dev, uint8_t* image_out, uint8_t* dir_out,
                 double* reward64_out, uint8_t* done_out, uint8_t* pixels_out, void* stream);

/* A step that logs its own tap rows.  bbai_step_tap_set lists the envs (host array, any order, no duplicates; count 0 clears); then
 * bbai_step_tapped = bbai_step + "bbai_tap_ids of the listed envs into these rows" (image_out uint8[count][147], dir_out uint8[count],
 * reward64_out double[count], done_out uint8[count]; log row k = env ids[k]) -- with the rows written by the stepping lanes themselves
 * wherever the step kernel leaves the final outputs behind (fused consume, in-place layout, auto_reset 0): no launch behind the step.  A
 * tap launch is 3 us + a dependent-launch gap, a quarter of a 65 536-env step; a logger that follows a few envs through every step
 * (bench.py's in-run parity check, a monitor) should not cost that.  Unfused auto-resetting steps (option consume_fused 0) get the
 * launch behind k_consume: same bytes either way (tests/test_gpu_parity.py::test_step_tapped_equals_step_plus_tap).  reward64 must not
 * be NULL here.  BBAI_ERR_STATE before bbai_step_tap_set. */
int bbai_step_tap_set(bbai_env* env, const int64_t* ids_host, int64_t count);
int bbai_step_tapped(bbai_env* env, const uint8_t* actions_dev, uint8_t* image_dev, uint8_t* dir_dev, float* reward_dev, double* reward64_dev,
                     uint8_t* done_dev, int auto_reset, uint8_t* image_out, uint8_t* dir_out, double* reward64_out, uint8_t* done_out, void* stream);

/* An open-loop rollout: T steps with NO host round trip in between.  actions_dev[T][n_envs] are resident on the device -- the
 * random-action rollouts the reference's own level test plays (babyai/levels/levelgen.py:522-527), a replayed demonstration, a
 * benchmark's pre-drawn action stream.  For t = 0 .. T-1 exactly what a caller's loop would enqueue:
 *     bbai_step(actions_dev + t * n_envs, ...)                       (auto_reset as in bbai_step)
 *     bbai_render(image_dev -> pixels_dev)                           when pixels_dev != NULL
 *     bbai_tap_ids(...) into log rows obs_row0 + t / row0 + t        when tap != NULL
 * image / dir / reward / reward64 / done (/ pixels) hold the LAST step's outputs on return; the tap log keeps every step of the listed
 * envs: image_out [rows][count][147], dir_out [rows][count], pixels_out [rows][pix_count][9408] indexed by obs_row0 + t (a caller
 * that stored the reset()'s observation in row 0 passes obs_row0 = 1), reward64_out / done_out [rows][count] indexed by row0 + t.
 * The per-step calls give the same bytes (tests/test_gpu_parity.py::test_rollout_entry_*).
 * Since round 6 the entry is also the fast path of open-loop stepping: with encoded observations (pixels_dev NULL), no token buffer,
 * and steps that move their finished envs on themselves (the default: fused consume / in-place layout; or auto_reset 0), ONE k_step
 * launch takes every step the current look-ahead window has left (up to 64 single-room / 96 maze ticks) -- an env's step touches only its own state, so a 64-env
 * block walks through the ticks on its own, no launch boundary and no dependent-launch gap (4-5 us: a third of a 65 536-env step) in
 * between; tick t reads actions_dev + t * n_envs.  A tap log is then written by the stepping lanes (bbai_step_tapped's mechanism): pass
 * ids_dev = NULL and count = the number of envs listed by bbai_step_tap_set (log row k = env ids[k]; pix_count 0).  A tap log WITH
 * ids_dev is a bbai_tap_ids launch behind every step and keeps one step per launch.  Option "rollout_multi" 0 (BBAI_ROLLOUT_MULTI=0):
 * one step per launch everywhere. */
typedef struct bbai_tap_log {
    int64_t count, pix_count;           /* envs listed / how many of the first listed ones also log pixels */
    const int64_t* ids_dev;             /* int64[count] env indices; NULL: the envs of bbai_step_tap_set (count must match) */
    uint8_t* image_out; uint8_t* dir_out; double* reward64_out; uint8_t* done_out; uint8_t* pixels_out;
    int64_t obs_row0, row0;
} bbai_tap_log;
int bbai_rollout(bbai_env* env, int T, const uint8_t* actions_dev, uint8_t* image_dev, uint8_t* dir_dev, float* reward_dev,
                 double* reward64_dev, uint8_t* done_dev, int auto_reset, uint8_t* pixels_dev, const bbai_tap_log* tap, void* stream);

/* Generalised advantage estimation of a rollout on the current device (the loop of babyai/rl/algos/base.py:196-202 as
 * one reverse scan per env).  All buffers float32, env-major [num_envs][num_frames] (the order base.py:207-232 flattens
 * experiences to); masks[p][i] = 1 - done before frame i, last_mask / last_value [num_envs] = the mask and the critic's
 * value after the last frame.  Writes advantage and returnn = value + advantage.  float32 in the reference's operation
 * order: bit-identical to its torch loop. */
int bbai_gae(int64_t num_envs, int num_frames, const float* rewards_dev, const float* values_dev, const float* masks_dev,
             const float* last_mask_dev, const float* last_value_dev, double discount, double gae_lambda,
             float* advantage_dev, float* returnn_dev, void* stream);

/* Demonstrations that stay on the device (babyai_amd/imitation.py DemoStore / DemoBatch).  Handle-free like bbai_gae: caller's
 * buffers, caller's stream, launched on the CURRENT device.  Every buffer that is read as images (the history chunks'
 * image arrays, src_image) must start 16-byte aligned in an allocation that is a multiple of 16 bytes long -- true of anything
 * hipMalloc returns: the kernels fetch the aligned 16-byte words around the bytes they need.
 *
 * bbai_demo_spans replaces the host scan of a rollout chunk (scripts/make_agent_demos.py:84-88,112-123: keep an episode iff
 * it ended done with reward > 0 and the bot did not crash, at most filter_steps long if that is non-zero; otherwise go on with the
 * stream's next level).  done / gave_up / reward are one bbai_bot_rollout call's outputs, [chunk][n]; g0 = the global step index of
 * row 0.  Carry per stream, updated in place: last_done int32[n] (global index of the latest episode end, -1 at first), open
 * uint8[n] (1 = still looking), span int32[n][2] (first and last global step of the first solved episode).  *open_count_dev
 * (8 bytes on the device, zeroed by the call) receives the number of streams still open. */
int bbai_demo_spans(int64_t n, int chunk, const uint8_t* done_dev, const uint8_t* gave_up_dev, const float* reward_dev, int64_t g0,
                    int filter_steps, int32_t* last_done_dev, uint8_t* open_dev, int32_t* span_dev, uint64_t* open_count_dev, void* stream);

/* The spans of a batch of streams -> flat demonstrations (what scripts/make_agent_demos.py:111-112 appends per episode, kept as
 * arrays): frames of stream k = rows offset[k] .. offset[k + 1] of image_out uint8[frames][147] / dir_out / action_out uint8[frames],
 * taken from history rows span[k][0] .. span[k][1]; tokens_out uint8[n][72] = the token row of the episode's first step.
 * chunks_dev: device table of the bbai_bot_rollout outputs that make up the history, chunk_steps rows [t][n] each (global step
 * g = row g % chunk_steps of chunk g / chunk_steps); offset_dev int64[n + 1] = exclusive prefix sum of the span lengths, frames =
 * offset[n].  Outputs 16-byte aligned. */
typedef struct bbai_demo_chunk { const uint8_t* image; const uint8_t* dir; const uint8_t* action; const uint8_t* tokens; } bbai_demo_chunk;
int bbai_demo_pack(int64_t n, int64_t frames, int chunk_steps, const bbai_demo_chunk* chunks_dev, const int32_t* span_dev,
                   const int64_t* offset_dev, uint8_t* image_out, uint8_t* dir_out, uint8_t* action_out, uint8_t* tokens_out, void* stream);

/* Expert demonstrations for LISTED seeds (babyai_amd/imitation.py DemoStore.collect_seeds).  The reference's
 * scripts/train_intelligent_expert.py:106-147 generate_demos(env_name, seeds) plays ONE episode per listed seed -- env.seed(seed);
 * env.reset() (:115-116), BotAgent acts until done (:121-133) -- and keeps it iff reward > 0 (:134-139); reward == 0 is logged and dropped
 * (:140-141), a bot exception skips the seed (:142-144).  Its caller grow_training_set (:150-176) asks for the seeds the learner failed on.
 * Here a POOL of n envs plays the list: after every bbai_bot_rollout chunk, bbai_demo_jobs finds the envs whose episode ended (the first done
 * row of the chunk's column), appends a record for every kept one -- gave_up == 0 and reward > 0 on that row -- and hands each of them the
 * next unplayed position of the list, as the fixed-length, -1-padded id / seed lists that bbai_reseed takes.
 *   job_dev int32[n]    in / out: the list position env i plays, -1 = idle;     start_dev int32[n]: the global step its episode began at
 *   job_seeds_dev       uint64[n_jobs], the list;     g0: global step index of the chunk's row 0 (episodes begin on a chunk's row 0 only)
 *   ids_out int64[n] / seeds_out uint64[n]: env i itself and its new seed where it claimed a job, ids_out = -1 everywhere else
 *   records_out int32[n][4]: (env, first step, length, job) of the episodes kept in this call, in no particular order
 *   counters_dev uint64[4]: [0] job cursor (in / out; the caller starts it at the number of jobs already handed out, it may end above
 *   n_jobs), [1] episodes finished so far (running total), [2] records and [3] their frames in THIS call (zeroed by the call). */
int bbai_demo_jobs(int64_t n, int chunk, const uint8_t* done_dev, const uint8_t* gave_up_dev, const float* reward_dev, int64_t g0, int32_t* job_dev,
                   int32_t* start_dev, const uint64_t* job_seeds_dev, int64_t n_jobs, int64_t* ids_out, uint64_t* seeds_out, int32_t* records_out,
                   uint64_t* counters_dev, void* stream);

/* bbai_demo_pack for a list of records of bbai_demo_jobs (what train_intelligent_expert.py:139 appends per kept seed): demo k = rows
 * records[k][1] .. + records[k][2] - 1 of stream records[k][0], and the history is a RING of ring_slots chunks of chunk_steps rows
 * [t][n_streams] each: global step g = row g % chunk_steps of table entry (g / chunk_steps) % ring_slots.  offset_dev int64[count + 1] =
 * exclusive prefix sum of the lengths, frames = offset[count].  Chunks and outputs aligned and padded as for bbai_demo_pack. */
int bbai_demo_pack_list(int64_t count, int64_t frames, int64_t n_streams, int chunk_steps, int ring_slots, const bbai_demo_chunk* chunks_dev,
                        const int32_t* records_dev, const int64_t* offset_dev, uint8_t* image_out, uint8_t* dir_out, uint8_t* action_out,
                        uint8_t* tokens_out, void* stream);

/* A list of demonstrations of a store -> one flat batch (babyai/imitation.py:226-251 without transform_demos' Python lists): demo
 * order_dev[b] of the store (offset_dev int64[D + 1], src_image / src_action) becomes frames dst_start_dev[b] .. dst_start_dev[b + 1]
 * (int64[count + 1], last entry = frames).  Batch form: action_out int64[frames], done_out uint8[frames] (1 on a demo's last frame),
 * mask_out float32[frames] (0 on its first), episode_ids_out int64[frames] (= b); dir8_out / action8_out NULL.  Store form (a
 * sub-store: the train / validation split): dir8_out / action8_out uint8[frames] and src_dir given, the four batch outputs NULL.
 * src_image and every output 16-byte aligned. */
int bbai_demo_batch(int64_t count, int64_t frames, const int64_t* order_dev, const int64_t* dst_start_dev, const int64_t* offset_dev,
                    const uint8_t* src_image, const uint8_t* src_dir, const uint8_t* src_action, uint8_t* image_out, int64_t* action_out,
                    uint8_t* done_out, float* mask_out, int64_t* episode_ids_out, uint8_t* dir8_out, uint8_t* action8_out, void* stream);

/* Per-kernel timing for measurements (bench.py's roofline): while enabled, every k_step / k_consume / k_render launch is
 * bracketed by a HIP event pair ON THE STREAM IT IS LAUNCHED ON; bbai_profile_read returns the summed milliseconds and the
 * launch counts in that order.  enable: 1 = start from zero, 2 = resume (totals kept), 0 = pause (totals stay readable).
 * Costs two event records per launch.  A bbai_rollout launch of k_step takes several steps: bbai_get_option "profile_step_ticks" =
 * the steps the bracketed k_step launches took. */
int bbai_profile(bbai_env* env, int enable);
int bbai_profile_read(bbai_env* env, double* ms_total /* [3] */, int64_t* launches /* [3] */);

/* Stream switching policy.  enable != 0: every reset / step / render / bot_act ends by recording the handle's completion
 * event on its own stream, and a call on another stream only waits for that event -- the previous stream is never
 * touched again and may have been destroyed.  Costs one event record per call (measured +3.4 us per step at 65 536 envs,
 * profiles/r03/call_events_ab.jsonl), hence off by default (BBAI_CALL_EVENTS=1 in the environment turns it on at create). */
int bbai_set_call_events(bbai_env* env, int enable);

/* The reference's done-action verifier mode (babyai/levels/verifier.py:17 `use_done_actions = os.environ.get(
 * 'BABYAI_DONE_ACTIONS', False)`, :216-230 ActionInstr.verify): an action instruction succeeds only on a `done` action taken
 * right after the step that completed it, and a `done` action at any other time FAILS it (episode over, reward 0).  A handle
 * starts in that mode iff the variable is non-empty in the environment at bbai_create -- the reference reads it at import --
 * and this call switches it explicitly (every env's lastStepMatch is cleared; call it between episodes).
 * AndInstr's extra failure rule (verifier.py:543-545: both of its instructions fail on a `done` => the And fails) sits behind
 * `action is self.env.actions.done`, an IDENTITY test: an int 6 never passes it (every vectorised caller of the reference steps
 * with ints, babyai/rl/utils/penv.py:8), the enum member does -- and the reference's own expert returns the member (babyai/bot.py:593,
 * fed to env.step by scripts/make_agent_demos.py:93-107).  A byte cannot carry that difference, so the caller says which it is:
 * bbai_bot_rollout applies the rule (its actions are the expert's), bbai_step applies it iff bbai_set_option(env,
 * "done_action_enum", 1) -- for a loop that steps with what bbai_bot_act suggested.  Pinned by traces of the reference stepped with
 * the enum member (tests/golden/done_actions_enum/, tests/test_done_actions.py).
 * The per-env bits travel in checkpoints; bbai_import_state clears them. */
int bbai_set_done_actions(bbai_env* env, int enable);
int bbai_get_done_actions(bbai_env* env);

/* Performance knobs of a live handle, by name (what the BBAI_* environment variables set at bbai_create; the reference has
 * no counterpart: these choose launch shapes and buffers, never results -- every setting but the last yields the same bytes, which
 * tests/test_gpu_parity.py::test_options_do_not_change_results checks).  Synchronises the device.  A knob's default and clamp are the same
 * whether its value comes from the variable at bbai_create or from a set (one table in bbai_engine.hip; tests/test_gpu_options.py).  Names:
 *   "render_queue"      -1 = by batch size (default), 0 = one-shot render blocks, m > 0 = persistent-block queue shape m
 *   "render_pace"       experiment: 1/16 ns of wall clock per render ticket (a time gate over two ticket counters); 0 = off (default)
 *   "render_queue_bpc", "render_queue_blocks"   persistent render blocks per CU (0 = 1024 threads' worth) / in total (0 = per CU)
 *   "render_group", "render_tpb"   envs / threads per one-shot render block (0 = by batch size)
 *   "render_delta"      1 (default; BBAI_RENDER_DELTA) = renders into the registered target store only changed lines
 *                       (bbai_set_render_target), 0 = full renders everywhere; setting it invalidates the target's history
 *   "render_target_tile_size"   8 (default), 16 or 32 (anything else: BBAI_ERR_ARG): the frame size of the NEXT bbai_set_render_target
 *                       registration, uint8[N][7 ts][7 ts][3] -- at 16 / 32 the target is bbai_render_view's
 *   "render_delta_sched", "render_delta_tpb", "render_delta_bpc"   the delta render's work split (0 = interleaved groups per
 *                       block, 1 = contiguous ranges, 2 as 0), threads per block (512 default / 1024) and blocks per CU (0 = 3 of 512
 *                       threads, 1 of 1024).  The store-only render behind a step that found the dirty cells, 64-byte pieces:
 *                       "render_delta_sched" 0 / 1 = groups handed out by a ticket counter, 2 = the static interleaved split (the
 *                       previous kernel, kept as the reference); "render_delta_bpc" 0 = 1 block per CU with the tickets, 3 without
 *   "step_prio", "pregen_group", "pregen_blocks", "pregen_min", "consume_fused"   as BBAI_STEP_PRIO / BBAI_PREGEN_GROUP /
 *                       BBAI_PREGEN_BLOCKS / BBAI_PREGEN_MIN / BBAI_CONSUME_FUSED
 *   "step_render_split" bbai_step_render / bbai_rollout with pixels: 1 = step the batch in two halves, the second under the first half's
 *                       render; 0 = never; -1 = the library's default
 *   "gate_strict"       1 = the step stream ALSO waits, at the start of every look-ahead window, for the refill launched two windows
 *                       earlier (rounds 1-4's rule); 0 (default) = it runs ahead of the refills as far as every env is sure to keep
 *                       a window's worth of ready levels (k_gate) -- a reset storm then refills under the steps
 *   "gate_probe"        1 (default; BBAI_GATE_PROBE) = the first window a caller's stream opens probes whether its kernels run concurrently with the
 *                       look-ahead stream's (HIP does not promise it: streams may share a hardware queue, a profiler may serialise
 *                       launches); a stream that fails runs under the strict rule.  0 = no probe, 2 = every probe fails (tests).  Setting
 *                       it forgets the verdicts so far
 *   "pregen_per_group"  single-room levels: list entries per working lane group of a refill launch (BBAI_PREGEN_PER_GROUP, default 12)
 *   "pregen_lane"       which kernel generates the look-ahead levels (results identical): 1 = k_pregen_lane, one lane per level (bit boards and an
 *                       object table instead of planes; every LevelGen parameterisation and the single-instruction levels without a lock-first
 *                       prologue; default for the single rooms), 0 = k_pregen, one lane group per level (every kind; default elsewhere);
 *                       BBAI_PREGEN_LANE at bbai_create.  Setting it converts the handle's MT19937 states between the two kernels' forms.
 *                       BBAI_ERR_ARG when 1 is asked of a kind the lane generator does not cover
 *   "lane_blocks"       upper bound on k_pregen_lane's waves per launch (BBAI_LANE_BLOCKS, default 16 384)
 *   "lookahead_streams" look-ahead streams a window's refill is split over (1 .. 8, default 1; BBAI_LOOKAHEAD_STREAMS): each takes a contiguous range of
 *                       64-env blocks, so an env's levels stay in stream order on ONE stream while the ranges' refills run side by side.  Measured: no gain
 *                       (a refill launch lasts as long as its slowest wave whatever its size) -- and the extra streams are created only while asked
 *                       for: every HIP stream is a hardware queue, a dozen per handle slow EVERY dispatch down
 *   "rollout_multi"     bbai_rollout with encoded observations: 1 (default; BBAI_ROLLOUT_MULTI) = one k_step launch per look-ahead window's remaining steps,
 *                       0 = one launch per step
 *   "gate_fault_inject" tests: raise (1) / clear (0) the sticky word a timed-out window gate leaves behind
 *   "bot_group"         the expert's kernel (bbai_bot_act / bbai_bot_rollout): 0 (default) = one lane per env (k_bot), 16 = one 16-lane
 *                       group per env with the first search in LDS (k_botg: same decisions, measured ~2 x slower -- an experiment
 *                       kept for reference); also BBAI_BOT_GROUP at bbai_create
 *   "done_action_enum"  a semantic switch (one of three in this list), meaningful in done-action mode only: see bbai_set_done_actions
 *   "step_hold"         the third semantic switch: 1 = action byte BBAI_ACTION_HOLD means "this env sits the step out" (see bbai_step), 0 (default) =
 *                       byte 8 is `done` like every unknown action; any non-zero value is stored as 1.  Read on the host when a stepping call is
 *                       enqueued, so setting it does not synchronise the device: a caller sets it around single calls of a running loop
 *   "reseed_levels"     the second semantic switch: how many levels of the new stream the following bbai_reseed calls generate per listed env (see
 *                       bbai_reseed).  0 (default), or anything >= the ring's depth: the whole ring.  Negative values are stored as 0.  Read on the
 *                       host when a bbai_reseed is enqueued, so setting it does not synchronise the device and costs no allocation
 * BBAI_ERR_ARG for an unknown name. */
int bbai_set_option(bbai_env* env, const char* name, int64_t value);
/* Read a knob back (the names of bbai_set_option), or "lookahead_period" (the refill period the handle chose at bbai_create), or
 * "inplace" (1: the in-place state layout, bbai_create), or "gate_timeouts" (synchronises: window gates that gave up waiting for a
 * look-ahead refill after ~10 s -- must be 0; anything else means a refill was lost and the batch's results are void), or
 * "gate_fault" (the same fact as a sticky flag in pinned host memory, read without synchronising: once it is set EVERY stepping /
 * resetting entry point of the handle returns BBAI_ERR_STATE before it enqueues anything, until bbai_seed regenerates the ring),
 * or "gate_forced_strict" (1: the caller's stream failed the concurrency probe and runs under the strict rule), or "owned" (how many
 * resources the handle holds right now -- device allocations, its pinned host words, streams and events: what bbai_destroy releases;
 * features that allocate on first use add to it once, not per call). */
int bbai_get_option(bbai_env* env, const char* name, int64_t* out);

/* Number of level generations (resets) performed so far, all envs. */
int bbai_reset_count(bbai_env* env, uint64_t* out);

/* Levels the generator gave up on (last-resort guard after 200 000 rejected attempts; the env is frozen).  Expected 0:
 * every unbounded rejection loop of the reference that can spin for ever is bounded explicitly. */
int bbai_generator_failures(bbai_env* env, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif
