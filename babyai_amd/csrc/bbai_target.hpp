// bbai_target.hpp -- the registered render target (bbai_set_render_target) as a record and one planner, for tile sizes 8, 16 and 32.
// Plain C++: no HIP, no device code (tests/test_render_target_host.py compiles it with g++ and drives it with made-up addresses).
//
// The caller registers ONE buffer uint8[n][7 ts][7 ts][3]; the handle keeps, in `shadow`, the atlas tile id of every cell of the frame the
// buffer holds.  While the shadow is valid, a render of target envs into their own rows stores only what changed (DELTA); while it is not,
// the same render draws the frames whole and writes every tile id behind them (FILL), and the shadow becomes valid once such fills have
// covered envs [0, n) in order.  Every other render (ELSEWHERE) that writes into the registered buffer leaves a frame the shadow does not
// describe and invalidates it; one that writes elsewhere leaves the target alone.  A render is three steps -- plan_target, the launches,
// commit_target -- and the state moves to what the plan promised only when the launches and the call's exit succeeded.
// Addresses are integers: the planner compares and offsets addresses of unrelated buffers, which is defined for integers and not for
// pointers.
#pragma once
#include <stdint.h>
#include "bbai_types.hpp"

namespace bbai {

constexpr int TARGET_ALIGN_8 = 128;       // a target at 8: the buffer on a 128-byte line (the delta render's LINE_BYTES, bbai_render.hpp) ...
constexpr int TARGET_UNIT_8 = 8;          // ... and a range starting on a line-aligned unit of envs (DELTA_UNIT: 8 x 9408 B)
constexpr int TARGET_ALIGN_VIEW = 64;     // a target at 16 / 32: the buffer on a 64-byte piece (VIEW_PIECE, bbai_viewpx.hpp)

struct RenderTarget {
    uintptr_t pixels = 0;         // the registered caller-owned uint8[n][7 ts][7 ts][3] buffer (0: none); only this handle's renders write there
    int ts = TILE;                // the tile size of that registration: 8 (bbai_render's delta render), 16 / 32 (bbai_render_view's: k_view_delta)
    uint8_t* shadow = nullptr;    // [n][49] tile id of every cell of the frame in `pixels`, in the atlas of `ts` (allocated at the first registration)
    uint64_t* dmask = nullptr;    // [n] the dirty-cell mask of every env, left by k_step for the store-only render (k_render_dstore); allocated with `shadow`
    bool valid = false;           // `shadow` describes `pixels`
    int64_t filled = 0;           // while not valid: envs [0, filled) rewritten by FILL renders since the last invalidation (a split render's halves)
    int64_t n = 0;                // envs of the batch
};

// One render: `nr` frames of tile size `ts` into the `bytes` bytes at `out`, for envs [env_off, env_off + nr) of the batch.
struct RenderRequest {
    int ts;
    uintptr_t out; int64_t bytes;
    int64_t env_off, nr;
    bool partial;                 // rows listed by id, or fewer rows than the batch (bbai_render_view; a tile-size-8 render has neither)
    bool delta;                   // option "render_delta" is on
};

struct TargetPlan {
    enum Kind { ELSEWHERE, FILL, DELTA } kind;
    int64_t shadow_off;           // FILL / DELTA: where the range's rows of the shadow start (env_off * 49)
    int64_t env_off, nr;          // the request's range (commit_target)
};

// The one place that writes this pair.
inline void invalidate_target(RenderTarget& t) { t.valid = false; t.filled = 0; }

// bbai_set_render_target (pixels 0: un-register; the shadow and the masks stay allocated)
inline void register_target(RenderTarget& t, uintptr_t pixels, int ts, int64_t n) {
    t.pixels = pixels; t.ts = ts; t.n = n;
    invalidate_target(t);
}

// The atlas of tile size `ts` was replaced: a frame registered at that size was drawn with the old one.
inline void target_atlas_replaced(RenderTarget& t, int ts) { if (t.ts == ts) invalidate_target(t); }

// Is the request a render of target envs into their own rows?  At 8 any range [env_off, env_off + nr) of the batch that starts on a unit
// (bbai_step_render's split halves), the buffer line-aligned; at 16 / 32 only the whole unlisted batch at the registered pointer, the buffer
// piece-aligned.  A render at another tile size, with "render_delta" 0 or before the shadow exists is never on target.
inline bool on_target(const RenderTarget& t, const RenderRequest& q) {
    if (!t.pixels || !t.shadow || q.ts != t.ts || !q.delta) return false;
    if (t.ts == TILE)
        return q.out == t.pixels + (uintptr_t)(q.env_off * PIX_BYTES) && q.env_off >= 0 && q.env_off + q.nr <= t.n &&
               t.pixels % TARGET_ALIGN_8 == 0 && q.env_off % TARGET_UNIT_8 == 0;
    return q.out == t.pixels && !q.partial && q.env_off == 0 && q.nr == t.n && t.pixels % TARGET_ALIGN_VIEW == 0;
}

// Do the request's bytes overlap the registered buffer (at whatever tile size it was registered: its true length)?
inline bool overlaps_target(const RenderTarget& t, const RenderRequest& q) {
    return t.pixels && q.out < t.pixels + (uintptr_t)(t.n * (int64_t)(OBS_BYTES * t.ts * t.ts)) && q.out + (uintptr_t)q.bytes > t.pixels;
}

// What the request means for the target.  ELSEWHERE into the registered buffer invalidates here and now; FILL and DELTA change nothing
// until commit_target.
inline TargetPlan plan_target(RenderTarget& t, const RenderRequest& q) {
    TargetPlan p = {TargetPlan::ELSEWHERE, 0, q.env_off, q.nr};
    if (!on_target(t, q)) {
        if (overlaps_target(t, q)) invalidate_target(t);
        return p;
    }
    p.kind = t.valid ? TargetPlan::DELTA : TargetPlan::FILL;
    p.shadow_off = q.env_off * (VIEW * VIEW);
    return p;
}

// A render that is never one of target envs into their own rows -- whole frames of another picture (bbai_render_view_pixels: any view size,
// atlases of its own), `bytes` bytes at `out`: a foreign write where it overlaps the registered buffer (tile size 0 is no registration's).
inline TargetPlan plan_foreign(RenderTarget& t, uintptr_t out, int64_t bytes) {
    return plan_target(t, RenderRequest{0, out, bytes, 0, 0, true, false});
}

// Would a tile-size-8 render of the whole batch into `pixels` be a DELTA render?  (bbai_step_render asks before its step kernel, which
// then finds the dirty cells for it; plans and changes nothing.)
inline bool whole_batch_delta(const RenderTarget& t, uintptr_t pixels, bool delta) {
    return t.valid && on_target(t, RenderRequest{TILE, pixels, t.n * (int64_t)PIX_BYTES, 0, t.n, false, delta});
}

// Behind the launches and the call's exit.  ok: a FILL of the range the fills have reached extends them, and the shadow is valid once they
// cover [0, n); a DELTA leaves it valid.  Not ok: the buffer or the shadow may hold part of a frame -- no shadow to trust.
inline void commit_target(RenderTarget& t, const TargetPlan& p, bool ok) {
    if (p.kind == TargetPlan::ELSEWHERE) return;
    if (!ok) { invalidate_target(t); return; }
    if (p.kind != TargetPlan::FILL) return;
    if (p.env_off == t.filled) t.filled = p.env_off + p.nr;
    if (t.filled >= t.n) t.valid = true;
}

}  // namespace bbai
