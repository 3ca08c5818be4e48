// bbai_target.hpp -- the handle's registered pixel buffers as ONE record type and one planner: the 7x7 view's target (bbai_set_render_target,
// tile sizes 8, 16 and 32) and the full-grid target (bbai_set_grid_target, include/bbai_grid_target.h).
// Plain C++: no HIP, no device code (tests/test_render_target_host.py, tests/test_grid_delta_host.py and tests/test_targets_host.py compile it
// with g++ and drive it with made-up addresses).
//
// The caller registers ONE buffer of n frames per target -- uint8[n][7 ts][7 ts][3], uint8[n][H ts][W ts][3] --; the handle keeps, in
// `shadow`, the atlas tile id of every cell of the frame the buffer holds.  While the shadow is valid, a render of target envs into their
// own rows stores only what changed (DELTA); while it is not, the same render draws the frames whole and writes every tile id behind them
// (FILL), and the shadow becomes valid once such fills have covered envs [0, n) in order.  EVERY other write of this handle into the
// registered bytes leaves a frame the shadow does not describe and invalidates it, here and now; one that lands elsewhere leaves the target
// alone.  That rule is written once: a frame-writing call announces its write through one of the three plan_target entries below -- a view
// render, a grid-target render, any other write --, each of which plans the target the write may be a render of and tells the other one
// (or both) the bytes; then come the launches, then commit_target, and the state moves to what the plan promised only when the launches and
// the call's exit succeeded.
// Addresses are integers: the planner compares and offsets addresses of unrelated buffers, which is defined for integers and not for
// pointers.
#pragma once
#include <stdint.h>
#include "bbai_types.hpp"

namespace bbai {

constexpr int TARGET_ALIGN_8 = 128;       // a view target at 8: the buffer on a 128-byte line (the delta render's LINE_BYTES, bbai_render.hpp) ...
constexpr int TARGET_UNIT_8 = 8;          // ... and a range starting on a line-aligned unit of envs (DELTA_UNIT: 8 x 9408 B)
constexpr int TARGET_ALIGN_VIEW = 64;     // a view target at 16 / 32: the buffer on a 64-byte piece (VIEW_PIECE, bbai_viewpx.hpp)
constexpr int GRID_TARGET_ALIGN = 64;     // the grid target: the buffer on a 64-byte piece (GRID_PIECE, bbai_gridtarget.hpp)

struct Target {
    uintptr_t pixels = 0;         // the registered caller-owned buffer of n frames (0: none); only this handle's renders write there
    int ts = TILE;                // the tile size of that registration
    uint8_t* shadow = nullptr;    // [n][cells of a frame] tile id of every cell of the frame in `pixels`, in the atlas of `ts` (allocated at the first registration)
    bool valid = false;           // `shadow` describes `pixels`
    int64_t filled = 0;           // while not valid: envs [0, filled) rewritten by FILL renders since the last invalidation (a split render's halves)
    int64_t n = 0;                // envs of the batch
    int64_t frame_bytes = 0;      // bytes of one frame: 147 ts^2 (view_frame_bytes), 3 W H ts^2 (grid_frame_bytes)
};
struct RenderTarget : Target {    // the 7x7 view's: ts 8 (bbai_render's delta render), 16 / 32 (bbai_render_view's: k_view_delta)
    uint64_t* dmask = nullptr;    // [n] the dirty-cell mask of every env, left by k_step for the store-only render (k_render_dstore); allocated with `shadow`
};
using GridTarget = Target;        // the full grid's: the shadow row-major y W + x, in the grid atlas of `ts`
struct Targets { RenderTarget view; GridTarget grid; };

inline int64_t view_frame_bytes(int ts) { return (int64_t)OBS_BYTES * ts * ts; }
inline int64_t grid_frame_bytes(int64_t cells, int ts) { return 3 * cells * ts * ts; }
inline int64_t target_bytes(const Target& t) { return t.n * t.frame_bytes; }       // the buffer's extent

// The one place that writes this pair.
inline void invalidate_target(Target& t) { t.valid = false; t.filled = 0; }

// bbai_set_render_target, bbai_set_grid_target (pixels 0: un-register; the shadow and the masks stay allocated).  The history starts invalid.
inline void register_target(Target& t, uintptr_t pixels, int ts, int64_t n, int64_t frame_bytes) {
    t.pixels = pixels; t.ts = ts; t.n = n; t.frame_bytes = frame_bytes;
    invalidate_target(t);
}

// The target's atlas of tile size `ts` was replaced: a frame registered at that size was drawn with the old one.
inline void target_atlas_replaced(Target& t, int ts) { if (t.ts == ts) invalidate_target(t); }

// Do the `bytes` bytes at `out` overlap the registered buffer (at whatever tile size it was registered: its true length)?  A range that
// ends where the buffer starts, or starts where it ends, does not; an empty one overlaps nothing.  The one place with this arithmetic:
// 64 bits throughout (buffers beyond 4 GiB).
inline bool overlaps_target(const Target& t, uintptr_t out, int64_t bytes) {
    return t.pixels && bytes > 0 && out < t.pixels + (uintptr_t)target_bytes(t) && out + (uintptr_t)bytes > t.pixels;
}
// A write that is no planned render of `t`: where it lands in the registered buffer the history is gone.
inline void foreign_write(Target& t, uintptr_t out, int64_t bytes) { if (overlaps_target(t, out, bytes)) invalidate_target(t); }

// ---- the three ways to announce a write, and the plan each returns ----------------------------------------------------------------------
// A view render: `nr` frames of tile size `ts` into the `bytes` bytes at `out`, for envs [env_off, env_off + nr) of the batch.
struct RenderRequest {
    int ts;
    uintptr_t out; int64_t bytes;
    int64_t env_off, nr;
    bool partial;                 // rows listed by id, or fewer rows than the batch (bbai_render_view; a tile-size-8 render has neither)
    bool delta;                   // option "render_delta" is on
};
// A render of the whole batch into the registered grid target (bbai_render_grid_target, bbai_step_grid_target).
struct GridRenderRequest { bool delta; };       // option "grid_render_delta" is on
// Any other write of frames or observations: `bytes` bytes at `out` (bbai_render_grid, bbai_render_view_pixels, bbai_observe_*, the
// frames of bbai_step_full / bbai_step_view).
struct WriteRequest { uintptr_t out; int64_t bytes; };

struct TargetPlan {
    enum Kind { ELSEWHERE, FILL, DELTA } kind;
    bool grid;                    // FILL / DELTA: of the grid target (else of the view's)
    int64_t shadow_off;           // FILL / DELTA: where the range's rows of the shadow start (env_off * 49; the grid's: 0)
    int64_t env_off, nr;          // the range (commit_target)
};

// The two "is this a render of target envs into their own rows?" rules, which really differ.
// The view's.  At 8 any range [env_off, env_off + nr) of the batch that starts on a unit (bbai_step_render's split halves), the buffer
// line-aligned; at 16 / 32 only the whole unlisted batch at the registered pointer, the buffer piece-aligned.  A render at another tile
// size, with "render_delta" 0 or before the shadow exists is never on target: it draws whole frames and writes no tile id (ELSEWHERE).
inline bool view_on_target(const RenderTarget& t, const RenderRequest& q) {
    if (!t.pixels || !t.shadow || q.ts != t.ts || !q.delta) return false;
    if (t.ts == TILE)
        return q.out == t.pixels + (uintptr_t)(q.env_off * PIX_BYTES) && q.env_off >= 0 && q.env_off + q.nr <= t.n &&
               t.pixels % TARGET_ALIGN_8 == 0 && q.env_off % TARGET_UNIT_8 == 0;
    return q.out == t.pixels && !q.partial && q.env_off == 0 && q.nr == t.n && t.pixels % TARGET_ALIGN_VIEW == 0;
}
// The grid's.  Its renders have no buffer argument -- always the whole batch at the registered pointer, which bbai_set_grid_target held to
// GRID_TARGET_ALIGN --, so every one is on target; with "grid_render_delta" 0 it is still a FILL, which writes the shadow and keeps it valid.
inline bool grid_on_target(const GridTarget& t, const GridRenderRequest&) { return t.pixels && t.shadow; }

// A view render plans the view target and tells the grid target its bytes.  ELSEWHERE into the registered buffer invalidates here and now;
// FILL and DELTA change nothing until commit_target.
inline TargetPlan plan_target(Targets& ts, const RenderRequest& q) {
    foreign_write(ts.grid, q.out, q.bytes);
    if (!view_on_target(ts.view, q)) {
        foreign_write(ts.view, q.out, q.bytes);
        return TargetPlan{TargetPlan::ELSEWHERE, false, 0, q.env_off, q.nr};
    }
    return TargetPlan{ts.view.valid ? TargetPlan::DELTA : TargetPlan::FILL, false, q.env_off * (VIEW * VIEW), q.env_off, q.nr};
}
// A grid-target render plans the grid target and tells the view target its bytes.
inline TargetPlan plan_target(Targets& ts, const GridRenderRequest& q) {
    if (!grid_on_target(ts.grid, q)) return TargetPlan{TargetPlan::ELSEWHERE, true, 0, 0, ts.grid.n};       // (nothing registered: nothing written)
    foreign_write(ts.view, ts.grid.pixels, target_bytes(ts.grid));
    return TargetPlan{ts.grid.valid && q.delta ? TargetPlan::DELTA : TargetPlan::FILL, true, 0, 0, ts.grid.n};
}
// Any other write tells both.
inline TargetPlan plan_target(Targets& ts, const WriteRequest& q) {
    foreign_write(ts.view, q.out, q.bytes);
    foreign_write(ts.grid, q.out, q.bytes);
    return TargetPlan{TargetPlan::ELSEWHERE, false, 0, 0, 0};
}

// Would a tile-size-8 render of the whole batch into `pixels` be a DELTA render?  (bbai_step_render asks before its step kernel, which
// then finds the dirty cells for it; plans and changes nothing.)
inline bool whole_batch_delta(const RenderTarget& t, uintptr_t pixels, bool delta) {
    return t.valid && view_on_target(t, RenderRequest{TILE, pixels, t.n * (int64_t)PIX_BYTES, 0, t.n, false, delta});
}

// Behind the launches and the call's exit, for the target the plan covered.  ok: a FILL of the range the fills have reached extends them,
// and the shadow is valid once they cover [0, n) (the grid's FILL is the whole batch: valid at once, and still valid where it was); a DELTA
// leaves it valid.  Not ok: the buffer or the shadow may hold part of a frame -- no shadow to trust.
inline void commit_target(Targets& ts, const TargetPlan& p, bool ok) {
    if (p.kind == TargetPlan::ELSEWHERE) return;
    Target& t = p.grid ? ts.grid : static_cast<Target&>(ts.view);
    if (!ok) { invalidate_target(t); return; }
    if (p.kind != TargetPlan::FILL) return;
    if (p.env_off == t.filled) t.filled = p.env_off + p.nr;
    if (t.filled >= t.n) t.valid = true;
}

}  // namespace bbai
