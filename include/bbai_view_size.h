#ifndef BBAI_VIEW_SIZE_H
#define BBAI_VIEW_SIZE_H
#include "bbai.h"
#ifdef __cplusplus
extern "C" {
#endif

/* bbai_view_size.h -- the view-size entries of libbbai_hip.so's C ABI: companion of bbai.h, which it includes (status codes, bbai_step and
 * its arguments).  The two entries stand next to bbai_observe_full / bbai_step_full in the library; they have a header of their own
 * because tests/test_binding_host.py pins the number of prototypes of bbai.h (as bbai_demo_replay.h's have).  babyai_amd/engine.py
 * ABI_VIEW is this header as ctypes sees it (tests/test_view_size_host.py holds the two against each other).
 *
 * The egocentric observation at another view size: gym-minigrid's ViewSizeWrapper(env, agent_view_size) -- RoomGridLevel passes
 * agent_view_size through to MiniGridEnv (babyai/levels/levelgen.py:25-33), the wrapper sets it on the unwrapped env and changes nothing
 * else -- on the device, for view_size V in 3, 5, 7, 9, 11.  A frame is uint8[V][V][3], image[vi][vj][channel],
 * the agent at view cell (V / 2, V - 1) facing up: the V x V window at get_view_exts() (a cell outside the grid is a wall), process_vis
 * from the agent's cell, the carried object on the agent's cell, an unseen cell 0, 0, 0.  "The observation" is what the wrapped env last
 * returned from reset() / step(): on the PutNext...Carrying levels an env that has not stepped yet shows the object still on its cell
 * and the agent's cell empty, as the reference's reset() does (bonus_levels.py:821-829).  At V = 7 the frames are the bytes bbai_step
 * writes.
 *
 * bbai_observe_view writes frame k = env ids_dev[k] (int64 device array; NULL = envs 0 .. count - 1) into out_dev + k * 3 V V (16-byte
 * aligned).  It reads the current state and writes nothing but out_dev; asynchronous on `stream`, ordered behind the handle's previous
 * calls.  An id outside [0, n) yields an all-zero frame; an id may be listed more than once.  BBAI_ERR_ARG for a null handle, a view size
 * outside the five, count < 0, count > n without ids, or a missing / misaligned out_dev; BBAI_ERR_STATE before the first reset.  A
 * refused call writes nothing.
 *
 * bbai_step_view (replaces ViewSizeWrapper(env, V).step for every env): bbai_step's launches, then the view of EVERY env of the state the
 * step leaves behind -- a finished env's next episode under auto_reset, a frozen env's final state without, a held env's unchanged one
 * (BBAI_ACTION_HOLD) -- into view_dev[n][V][V][3] (16-byte aligned), as ONE call.  image_dev (the 7x7 view) and the other outputs are
 * written as by bbai_step.  The device expert (bbai_bot_act, bbai_bot_rollout) keeps its 7x7 visibility whatever is observed here. */
int bbai_observe_view(bbai_env* env, int view_size, const int64_t* ids_dev /* NULL = envs 0..count-1 */, int64_t count,
                      uint8_t* out_dev /* [count][V][V][3] */, void* stream);
int bbai_step_view(bbai_env* env, const uint8_t* actions_dev, uint8_t* image_dev, uint8_t* dir_dev, float* reward_dev,
                   double* reward64_dev, uint8_t* done_dev, int auto_reset, int view_size, uint8_t* view_dev /* [n][V][V][3] */,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
