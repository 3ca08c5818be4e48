#ifndef BBAI_VIEW_PIXELS_H
#define BBAI_VIEW_PIXELS_H
#include "bbai.h"
#ifdef __cplusplus
extern "C" {
#endif

/* bbai_view_pixels.h -- the partial-view pixel entries for any view size of libbbai_hip.so's C ABI: companion of bbai.h, which it includes
 * (status codes, bbai_env).  The two entries stand next to bbai_set_view_atlas / bbai_render_view in the library; they have a header of
 * their own because tests/test_binding_host.py pins the number of prototypes of bbai.h (as bbai_demo_replay.h's and bbai_view_size.h's
 * have).  babyai_amd/engine.py ABI_VIEW_PIXELS is this header as ctypes sees it (tests/test_view_pixels_host.py holds the two against
 * each other).
 *
 * The picture: gym_minigrid's RGBImgPartialObsWrapper(ViewSizeWrapper(env, V), tile_size).observation -- the wrapper calls
 * MiniGridEnv.get_obs_render(obs['image'], tile_size), which decodes the V x V encoding into a grid and renders it with the agent at
 * (V // 2, V - 1) facing up, for whatever agent_view_size the env has -- for view_size V in 3, 5, 7, 9, 11 and tile_size 8, 16, 32
 * (DESIGN.md section 5m).  A frame is uint8[V ts][V ts][3]: pixel [row = vj * ts + y][column = vi * ts + x] is pixel (y, x) of the tile
 * of view cell (vi, vj), whose encoding is image[vi][vj] = (o0, o1, o2).  The tile is lut[cell == agent cell][key] of the atlas, key =
 * (o0 | o1 << 3 | o2 << 6) & 255, the agent's cell being (V // 2, V - 1) -- index (V // 2) * V + V - 1 = 5, 14, 27, 44, 65; row 1 of the
 * lut draws what the agent carries with the agent's triangle over it.  A tile's picture does not depend on the view size: the atlases
 * are those of the 7x7 view (tools/gen_atlas.py).
 *
 * bbai_set_view_pixels_atlas installs the atlas of one tile size for bbai_render_view_pixels: tiles_host[n_tiles][ts][ts][3], n_tiles in
 * 1 .. 64, and lut_host[2][256] with every entry < n_tiles (both copied; host pointers).  The handle keeps these atlases apart from
 * bbai_set_atlas' and bbai_set_view_atlas': installing one here changes no other render and never touches a registered render target's
 * history.  It waits for the device (a render in flight may read the atlas being replaced).  BBAI_ERR_ARG for a null handle or pointer,
 * a tile size outside 8 / 16 / 32, a tile count out of range or a lut entry that names a tile the atlas does not hold; a refused call
 * installs nothing.
 *
 * bbai_render_view_pixels draws frame k = row ids_dev[k] (int64 device array; NULL = rows 0 .. count - 1) of the encoded buffer
 * image_dev[rows][V][V][3] into out_dev + k * 3 V V ts ts (16-byte aligned; a frame is a multiple of 64 bytes at every size).  It writes
 * nothing but out_dev; asynchronous on `stream`, ordered behind the handle's previous calls.  A row id outside [0, rows) yields an
 * all-zero frame and no read outside the buffer; an id may be listed more than once.  Where the frames overlap a registered buffer
 * (bbai_set_render_target, bbai_set_grid_target) they are a foreign whole-frame write: that target's history is invalidated, as by a
 * bbai_render_view with ids (the one list: bbai.h, bbai_set_render_target); a write elsewhere leaves both alone.  BBAI_ERR_ARG for a null handle, a view size or tile size outside the sets, rows < 0,
 * count < 0, count > rows without ids, a missing or misaligned out_dev, or a missing image_dev with work to do; BBAI_ERR_STATE while no
 * atlas of that tile size is installed; count == 0 is BBAI_OK.  A refused call writes nothing. */
int bbai_set_view_pixels_atlas(bbai_env* env, int tile_size /* 8|16|32 */, const uint8_t* tiles_host, int n_tiles /* <= 64 */,
                               const uint8_t* lut_host /* [2][256] */);
int bbai_render_view_pixels(bbai_env* env, int view_size /* 3|5|7|9|11 */, int tile_size /* 8|16|32 */,
                            const uint8_t* image_dev /* [rows][V][V][3], indexed [vi][vj] */, int64_t rows,
                            const int64_t* ids_dev /* NULL = rows 0..count-1 */, int64_t count,
                            uint8_t* out_dev /* [count][V*ts][V*ts][3], 16-byte aligned */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
