#ifndef BBAI_DEMO_REPLAY_H
#define BBAI_DEMO_REPLAY_H
#include "bbai.h"
#ifdef __cplusplus
extern "C" {
#endif

/* bbai_demo_replay.h -- the replay entries of libbbai_hip.so's C ABI: companion of bbai.h, which it includes (status codes,
 * BBAI_ACTION_HOLD, bbai_step, bbai_reseed, bbai_demo_jobs).  The two entries stand next to bbai_demo_jobs in the library; they have a
 * header of their own because tests/test_binding_host.py pins the number of prototypes of bbai.h.  babyai_amd/engine.py ABI_REPLAY is
 * this header as ctypes sees it (tests/test_demo_replay_abi.py holds the two against each other).
 *
 * Replay a demo store on the device (babyai_amd/imitation.py DemoStore.replay).  The reference's DemoAgent
 * (babyai/utils/agent.py:101-137) plays ONE demonstration back in one env -- act() returns the recorded action and asserts that the env
 * shows the recorded mission, image and direction (:118-133) -- and scripts/evaluate.py:45-57 builds `--demos` evaluation on it, seed by
 * seed (evaluate_demo_agent logs the demos' lengths: a demo holds no rewards).  Here a POOL of n envs (auto_reset = 0, option "step_hold"
 * = 1, a token buffer) plays the store's non-empty demos, one TICK = bbai_demo_replay_feed, bbai_step with the actions it wrote,
 * bbai_demo_replay_judge -- and, on the ticks the caller claims on, bbai_reseed(ids_out, seeds_out) under option "reseed_levels" = 1.  A
 * mismatch is counted, not fatal: the recorded actions go on being applied, and frames behind `done` are never compared.
 * Handle-free like bbai_demo_jobs: caller's buffers, caller's stream, launched on the CURRENT device.
 *
 * Pool state, in / out of both entries: job_dev int32[n] = the demo env i plays, < 0 = none (idle, or WAITING for the next claim: the two
 * are one state); pos_dev int32[n] = the frame of it the env stands at.  The store: offset_dev int64[n_demos + 1], store_image
 * uint8[frames][147], store_dir / store_action uint8[frames], store_tokens uint8[n_demos][72].  store_image and image_dev are read as
 * images under bbai.h's contract for those: 16-byte aligned start, allocation a multiple of 16 bytes; the token rows are read as 8-byte
 * pieces (8-byte aligned start).  Per-demo results, caller-initialised (mismatches 0, first_mismatch -1, the others 0): a demo's entries
 * are written by the one env that plays it.
 *
 * bbai_demo_replay_feed, before the step: env i is FED iff 0 <= job < n_demos, 0 <= pos < the demo's length and the frame offset[job] +
 * pos lies in [0, frames) -- no other job or pos is ever turned into an address.  A fed env's rows of image_dev [n][147] / dir_dev [n] are
 * compared with that frame: a difference adds 1 to mismatches[job] and sets first_mismatch[job] = pos while that is < 0; at pos == 0 its
 * row of tokens_dev [n][72] is compared with the demo's and mission_ok[job] = 1 / 0 written; actions_out[i] = the recorded action,
 * fed_out[i] = 1.  Every other env: actions_out[i] = BBAI_ACTION_HOLD, fed_out[i] = 0, results untouched.  Which envs were fed is kept
 * in fed_out uint8[n], an array of its own (no bit in job or pos): bbai_demo_replay_judge reads it and nothing else writes it. */
int bbai_demo_replay_feed(int64_t n, const uint8_t* image_dev, const uint8_t* dir_dev, const uint8_t* tokens_dev, const int32_t* job_dev,
                          const int32_t* pos_dev, int64_t n_demos, int64_t frames, const int64_t* offset_dev, const uint8_t* store_image,
                          const uint8_t* store_dir, const uint8_t* store_action, const uint8_t* store_tokens, int32_t* mismatches_dev,
                          int32_t* first_mismatch_dev, uint8_t* mission_ok_dev, uint8_t* actions_out, uint8_t* fed_out, void* stream);

/* bbai_demo_replay_judge, behind the step: acts on the envs with fed_dev[i] != 0 ONLY -- a held env's done_dev / reward64_dev entries are
 * stale by the HOLD contract, and a reseeded env's done_dev still reads 1 until its first real step.  A fed env's pos advances; with
 * done_dev[i] set, done_at[job] = played[job] = pos and return64[job] = reward64_dev[i], bit for bit; with the demo used up and no done,
 * played[job] = pos, done_at[job] = 0, return64[job] = 0.0; either way the env goes waiting (job = -1).  claim != 0: every env with job < 0,
 * those that finished in this call included, claims the next position k of the job list as bbai_demo_jobs hands positions out (one
 * returning add per wave): k < n_jobs gives job = job_demo_dev[k] (k itself with job_demo_dev NULL), pos = 0, ids_out[i] = i and
 * seeds_out[i] = job_seeds_dev[k] (uint64[n_jobs]); every other env gets ids_out[i] = -1 -- the fixed-length, -1-padded lists that
 * bbai_reseed takes.  claim == 0: nothing is claimed, ids_out / seeds_out are not touched (and may be NULL).  counters_dev uint64[2]:
 * [0] the job cursor (in / out: the caller starts it at the number of jobs already handed out; it may end above n_jobs), [1] demos
 * finished so far (running total).
 * Both entries: BBAI_ERR_ARG (before any launch) for n < 0, n_demos or frames < 1, n_jobs < 0, any count beyond 2^31 - 1 and, with n > 0,
 * a null or misaligned pointer; n == 0 is a no-op. */
int bbai_demo_replay_judge(int64_t n, const uint8_t* fed_dev, const uint8_t* done_dev, const double* reward64_dev, int32_t* job_dev,
                           int32_t* pos_dev, int64_t n_demos, const int64_t* offset_dev, int32_t* played_dev, int32_t* done_at_dev,
                           double* return64_dev, int claim, const int32_t* job_demo_dev, const uint64_t* job_seeds_dev, int64_t n_jobs,
                           int64_t* ids_out, uint64_t* seeds_out, uint64_t* counters_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
