#ifndef BBAI_GRID_TARGET_H
#define BBAI_GRID_TARGET_H
#include "bbai.h"
#ifdef __cplusplus
extern "C" {
#endif

/* bbai_grid_target.h -- the registered full-grid target of libbbai_hip.so's C ABI: companion of bbai.h, which it includes (status codes,
 * bbai_env).  The five entries stand next to bbai_set_grid_atlas / bbai_render_grid in the library; they have a header of their own
 * because tests/test_binding_host.py pins the number of prototypes of bbai.h (as bbai_view_pixels.h's have).  babyai_amd/engine.py
 * ABI_GRID_TARGET is this header as ctypes sees it (tests/test_grid_delta_host.py holds the two against each other).
 *
 * The picture: gym_minigrid's RGBImgObsWrapper(env, tile_size).observation -- env.render('rgb_array', highlight=False, tile_size) of the
 * whole grid (restated in oracle/shim/gym_minigrid/wrappers.py) -- for every env of the batch: a frame is uint8[H ts][W ts][3], exactly
 * the bytes bbai_render_grid(tile_size, highlight = 0) draws.  Between two steps almost none of them change (a turn changes one cell, a
 * move or an object action two, only a reset the whole grid), so the handle can keep ONE caller-owned buffer of frames current by
 * storing only the 64-byte pieces that hold a changed cell.
 *
 * bbai_set_grid_target registers frames_dev, uint8[n][H ts][W ts][3] on the handle's device, as that buffer (NULL un-registers); the
 * caller keeps it alive while it is registered and lets only this handle write it.  With the first registration the handle allocates
 * its shadow, uint8[n][W H]: the grid-atlas tile id of every cell of the frame the buffer holds, row-major y W + x.  A registration
 * starts with no history: the next render draws every frame whole.  BBAI_ERR_ARG for a null handle, a tile size outside 8 / 16 / 32 or
 * a buffer that is not 64-byte aligned; a refused call registers nothing.
 *
 * bbai_render_grid_target draws the current state of every env into the registered buffer, asynchronous on `stream`, ordered behind the
 * handle's previous calls (bbai_render_grid's conventions).  While the history is valid and option "grid_render_delta" (default 1) is
 * non-zero it is a delta render: the new tile ids are compared with the shadow, the changed ones written back, and exactly the 64-byte
 * pieces that hold bytes of a changed cell are stored -- not one byte of any other piece.  Otherwise it draws whole frames and fills
 * the shadow; either way the history is valid afterwards (read-only option "grid_delta_valid").  BBAI_ERR_STATE while no target is
 * registered, while no grid atlas of its tile size is installed (bbai_set_grid_atlas), and before reset.
 *
 * bbai_step_grid_target is bbai_step -- the same arguments, the same launches -- with that render behind it, as one call:
 * RGBImgObsWrapper's step.  BBAI_ERR_ARG for a null handle or buffer; BBAI_ERR_STATE as the render's and the step's.
 *
 * What drops the history: the one list of bbai.h (bbai_set_render_target), which holds for both registered buffers -- a registration,
 * bbai_set_grid_atlas at the registered tile size, bbai_grid_target_invalidate (call it after writing into the buffer yourself), a
 * render that failed, and every entry of this handle that writes frames or observations into a per-call buffer whose bytes overlap the
 * registered ones (bbai_render, bbai_step_render, bbai_render_view, bbai_render_view_pixels, bbai_render_grid, bbai_observe_full,
 * bbai_observe_view, the frames of bbai_step_full / bbai_step_view).  Likewise a grid target laid over the buffer registered with
 * bbai_set_render_target drops that one's history with every render.  State changes that never touch the buffer (bbai_load_state,
 * bbai_reseed, bbai_import_state, bbai_checkpoint_load) need nothing: the shadow describes the buffer, not the state, and the next
 * render compares.
 *
 * Option "grid_delta_group" (default 0): envs a block of the delta render works on at a time; 0 = chosen by batch size, a value above
 * what the kernel's planes hold for the grid is clamped.  Never semantics: every setting stores the same bytes (the tests run them all).
 *
 * bbai_grid_target_shadow copies the shadow into out_dev, uint8[n][W H], asynchronous on `stream`; BBAI_ERR_STATE before the first
 * registration. */
int bbai_set_grid_target(bbai_env* env, uint8_t* frames_dev /* [n][H*ts][W*ts][3], 64-byte aligned; NULL un-registers */, int tile_size /* 8|16|32 */);
int bbai_render_grid_target(bbai_env* env, void* stream);
int bbai_step_grid_target(bbai_env* env, const uint8_t* actions_dev, uint8_t* image_dev, uint8_t* direction_dev, float* reward_dev,
                          double* reward64_dev /* may be NULL */, uint8_t* done_dev, int auto_reset, void* stream);
int bbai_grid_target_invalidate(bbai_env* env);
int bbai_grid_target_shadow(bbai_env* env, uint8_t* out_dev /* [n][W*H] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
