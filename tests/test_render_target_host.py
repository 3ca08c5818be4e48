"""The registered render target's bookkeeping (babyai_amd/csrc/bbai_target.hpp: RenderTarget, plan_target, commit_target -- the view render's and the other write's entries) without a GPU:
the header compiled with g++ from a wrapper this test writes, driven with made-up addresses.  What a render means for the target --
ELSEWHERE, FILL or DELTA --, what invalidates the shadow and when it becomes valid again are checked against a model written here from
the contract in include/bbai.h (bbai_set_render_target, bbai_render_view), over an enumerated grid of targets and requests; then the call
sequences of four GPU tests that read "render_delta_valid" are replayed as planner calls and must give the same 0 / 1 sequence."""
import ctypes
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "babyai_amd", "csrc")
ELSEWHERE, FILL, DELTA = 0, 1, 2
N = 24                        # three units of 8 envs: halves of 8 and 16 exist
BASE = 0x7F0000000000         # 128-byte aligned; + 16 loses the 128-byte line (a target at 8) and the 64-byte piece (at 16 / 32)
FAR = 0x100000000000          # buffers that are not the registered one

WRAPPER = """
#include "bbai_target.hpp"
using namespace bbai;
static Targets g_both;                    // (the grid target stays un-registered: these tests are about the view's)
static RenderTarget& g = g_both.view;
static TargetPlan g_plan;
extern "C" {
void tg_new() { g_both = Targets(); }
// bbai_set_render_target: the shadow and the masks come with the first registration (addresses nobody reads)
void tg_register(unsigned long long pixels, int ts, long long n) {
    if (pixels && !g.shadow) { g.shadow = reinterpret_cast<uint8_t*>(uintptr_t(1) << 20); g.dmask = reinterpret_cast<uint64_t*>(uintptr_t(1) << 21); }
    register_target(g, (uintptr_t)pixels, ts, n, view_frame_bytes(ts));
}
void tg_invalidate() { invalidate_target(g); }
void tg_atlas_replaced(int ts) { target_atlas_replaced(g, ts); }
void tg_force(int valid, long long filled) { g.valid = valid != 0; g.filled = filled; }      // (the grid's "state beforehand")
int tg_plan(int ts, unsigned long long out, long long bytes, long long env_off, long long nr, int partial, int delta) {
    g_plan = plan_target(g_both, RenderRequest{ts, (uintptr_t)out, bytes, env_off, nr, partial != 0, delta != 0});
    return g_plan.kind == TargetPlan::ELSEWHERE ? 0 : g_plan.kind == TargetPlan::FILL ? 1 : 2;
}
long long tg_shadow_off() { return g_plan.shadow_off; }
void tg_commit(int ok) { commit_target(g_both, g_plan, ok != 0); }
int tg_query(unsigned long long pixels, int delta) { const RenderTarget& c = g; return whole_batch_delta(c, (uintptr_t)pixels, delta != 0) ? 1 : 0; }
int tg_foreign(unsigned long long out, long long bytes) { g_plan = plan_target(g_both, WriteRequest{(uintptr_t)out, bytes}); return g_plan.kind == TargetPlan::ELSEWHERE ? 0 : 1; }
int tg_valid() { return g.valid ? 1 : 0; }
long long tg_filled() { return g.filled; }
void tg_state(unsigned long long* s) {
    s[0] = g.pixels; s[1] = (unsigned long long)g.ts; s[2] = (uintptr_t)g.shadow; s[3] = (uintptr_t)g.dmask; s[4] = g.valid; s[5] = (unsigned long long)g.filled;
    s[6] = (unsigned long long)g.n;
}
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("render_target_host")
    src, so = str(d / "wrapper.cpp"), str(d / "librendertarget.so")
    with open(src, "w") as f:
        f.write(WRAPPER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I", CSRC, "-o", so, src])
    lib = ctypes.CDLL(so)
    U, L, I = ctypes.c_ulonglong, ctypes.c_longlong, ctypes.c_int
    for name, res, args in (("tg_new", None, []), ("tg_register", None, [U, I, L]), ("tg_invalidate", None, []), ("tg_atlas_replaced", None, [I]),
                            ("tg_force", None, [I, L]), ("tg_plan", I, [I, U, L, L, L, I, I]), ("tg_shadow_off", L, []), ("tg_commit", None, [I]),
                            ("tg_query", I, [U, I]), ("tg_foreign", I, [U, L]), ("tg_valid", I, []), ("tg_filled", L, []), ("tg_state", None, [ctypes.POINTER(U)])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def frame(ts):
    return 147 * ts * ts


def state(lib):
    s = (ctypes.c_ulonglong * 7)()
    lib.tg_state(s)
    return tuple(s)


# ---- A. properties over the grid ----------------------------------------------------------------------------------------------------
TARGETS = (None, 8, 16, 32)
REQUESTS = (8, 16, 32)
RANGES = ((0, N), (0, 8), (8, 16), (16, 8), (4, 8), (0, N + 8))


def offsets(target_ts, req_ts, env_off):
    """Output offsets from the buffer's start (a buffer of N frames of the target's size; with no target: of the request's)."""
    ft = frame(target_ts or req_ts)
    end = N * ft
    # (the last one: the exact rows of the range's first env, which the list above reaches only for env 0 and, at 8, env 8)
    return sorted({-frame(req_ts), -16, 0, 16, 8 * frame(8), ft, end - 16, end, end + ft, env_off * ft})


def grid():
    for target, req, (env_off, nr), listed, delta, aligned, valid in itertools.product(TARGETS, REQUESTS, RANGES, (0, 1), (0, 1), (1, 0), (0, 1)):
        if target is None and valid:
            continue                  # (no registration: nothing to be valid)
        for off in offsets(target, req, env_off):
            yield target, req, env_off, nr, listed, delta, aligned, valid, off


def setup(lib, target, aligned, valid):
    """The state beforehand -> the registered address."""
    base = BASE + (0 if aligned else 16)
    lib.tg_new()
    if target is not None:
        lib.tg_register(base, target, N)
        lib.tg_force(valid, 0)
    return base


def request(lib, req, out, env_off, nr, listed, delta):
    """As the engine words it: bbai_render_view's rows are partial when listed or fewer than the batch; bbai_render has neither notion."""
    partial = listed or (req != 8 and nr != N)
    return lib.tg_plan(req, out, nr * frame(req), env_off, nr, 1 if partial else 0, delta)


def model(target, req, env_off, nr, listed, delta, aligned, off):
    """From include/bbai.h: (the request's bytes intersect the registered buffer, the request is a render of target envs into their rows)."""
    if target is None:
        return False, False
    lo, hi = 0, N * frame(target)
    intersects = off < hi and off + nr * frame(req) > lo
    rows = off == env_off * frame(target) and env_off >= 0 and env_off + nr <= N
    on = bool(delta) and req == target and rows and bool(aligned) and env_off % 8 == 0
    if target != 8:
        on = on and not listed and env_off == 0 and nr == N
    return intersects, on


def test_grid_plan_and_successful_commit(lib):
    cases = 0
    for target, req, env_off, nr, listed, delta, aligned, valid, off in grid():
        case = (target, req, env_off, nr, listed, delta, aligned, valid, off)
        base = setup(lib, target, aligned, valid)
        before = state(lib)
        kind = request(lib, req, base + off, env_off, nr, listed, delta)
        intersects, on = model(target, req, env_off, nr, listed, delta, aligned, off)
        assert not on or intersects, case
        if not intersects:                                   # 1
            assert kind == ELSEWHERE and state(lib) == before, case
        elif not on:                                         # 3
            assert kind == ELSEWHERE and lib.tg_valid() == 0 and lib.tg_filled() == 0, case
        elif valid:                                          # 2
            assert kind == DELTA and state(lib) == before, case
        else:                                                # 4
            assert kind == FILL and lib.tg_shadow_off() == env_off * 49 and state(lib) == before, case
        assert (kind == DELTA) == (on and bool(valid)), case
        if not delta:                                        # 6: "render_delta" 0 -- every render is a full one
            assert kind == ELSEWHERE, case
        planned = state(lib)
        lib.tg_commit(1)
        if kind == DELTA:
            assert state(lib) == before and lib.tg_valid() == 1, case
        elif kind == FILL:
            covered = env_off == 0 and nr == N
            assert lib.tg_valid() == (1 if covered else 0) and lib.tg_filled() == (nr if env_off == 0 else 0), case
        else:
            assert state(lib) == planned, case
        cases += 1
    assert cases >= 7 * 3 * 6 * 8 * 9      # (targets x states) x requests x ranges x (listed, delta, aligned), each at nine offsets or ten


def test_grid_failed_commit(lib):                            # 5
    for target, req, env_off, nr, listed, delta, aligned, valid, off in grid():
        case = (target, req, env_off, nr, listed, delta, aligned, valid, off)
        base = setup(lib, target, aligned, valid)
        kind = request(lib, req, base + off, env_off, nr, listed, delta)
        planned = state(lib)
        lib.tg_commit(0)
        if kind == ELSEWHERE:
            assert state(lib) == planned, case
        else:
            assert lib.tg_valid() == 0 and lib.tg_filled() == 0, case


def test_fills_make_the_shadow_valid_once_they_cover_the_batch_in_order(lib):          # 4
    def fills(ts, seq):
        base = setup(lib, ts, 1, 0)
        for env_off, nr in seq:
            assert request(lib, ts, base + env_off * frame(ts), env_off, nr, 0, 1) == FILL, (ts, seq)
            assert lib.tg_shadow_off() == env_off * 49
            lib.tg_commit(1)
        return lib.tg_valid()
    assert fills(8, [(0, 8), (8, 16)]) == 1
    assert fills(8, [(8, 16), (0, 8)]) == 0
    assert fills(8, [(0, 8), (0, 8)]) == 0
    assert fills(8, [(0, 8)]) == 0
    assert fills(8, [(0, N)]) == 1
    assert fills(8, [(0, 16), (16, 8)]) == 1
    assert fills(16, [(0, N)]) == 1 and fills(32, [(0, N)]) == 1
    # a failed fill in between starts the count again; the next render of a valid shadow is a DELTA
    base = setup(lib, 8, 1, 0)
    assert request(lib, 8, base, 0, 8, 0, 1) == FILL
    lib.tg_commit(1)
    assert request(lib, 8, base + 8 * frame(8), 8, 16, 0, 1) == FILL
    lib.tg_commit(0)
    assert lib.tg_valid() == 0 and lib.tg_filled() == 0
    assert request(lib, 8, base + 8 * frame(8), 8, 16, 0, 1) == FILL
    lib.tg_commit(1)
    assert lib.tg_valid() == 0
    for env_off, nr in ((0, 8), (8, 16)):
        assert request(lib, 8, base + env_off * frame(8), env_off, nr, 0, 1) == FILL
        lib.tg_commit(1)
    assert lib.tg_valid() == 1
    assert request(lib, 8, base, 0, 8, 0, 1) == DELTA


@pytest.mark.parametrize("ts", [8, 16, 32])
def test_what_invalidates(lib, ts):                          # 6
    other = {8: 16, 16: 32, 32: 8}[ts]

    def valid_target():
        base = setup(lib, ts, 1, 0)
        assert request(lib, ts, base, 0, N, 0, 1) == FILL
        lib.tg_commit(1)
        assert lib.tg_valid() == 1 and lib.tg_filled() == N
        return base
    events = {"register": lambda b: lib.tg_register(b, ts, N), "register elsewhere": lambda b: lib.tg_register(FAR, ts, N),
              "unregister": lambda b: lib.tg_register(0, ts, N), "bbai_render_invalidate": lambda b: lib.tg_invalidate(),
              "the target's atlas replaced": lambda b: lib.tg_atlas_replaced(ts),
              "render_delta set (to 0 or to 1: the option's setter)": lambda b: lib.tg_invalidate()}
    for what, ev in events.items():
        ev(valid_target())
        assert lib.tg_valid() == 0 and lib.tg_filled() == 0, what
    for t in (8, 16, 32):
        valid_target()
        lib.tg_atlas_replaced(t)
        assert lib.tg_valid() == (0 if t == ts else 1), t
    # un-registered: no render is on target, none touches the state
    base = valid_target()
    lib.tg_register(0, ts, N)
    before = state(lib)
    assert request(lib, ts, base, 0, N, 0, 1) == ELSEWHERE and state(lib) == before
    # "render_delta" 0: the render of the target's own rows is a full render into the buffer
    base = valid_target()
    assert request(lib, ts, base, 0, N, 0, 0) == ELSEWHERE and lib.tg_valid() == 0 and lib.tg_filled() == 0
    # ... and at another tile size
    base = valid_target()
    assert request(lib, other, base, 0, N, 0, 1) == ELSEWHERE and lib.tg_valid() == 0


def test_the_query_changes_nothing_and_agrees_with_the_planner(lib):          # 7
    asked = 0
    for target, aligned, valid, delta in itertools.product(TARGETS, (1, 0), (0, 1), (0, 1)):
        if target is None and valid:
            continue
        for off in offsets(target, 8, 0):
            base = setup(lib, target, aligned, valid)
            before = state(lib)
            got = lib.tg_query(base + off, delta)
            assert state(lib) == before
            assert got == (1 if request(lib, 8, base + off, 0, N, 0, delta) == DELTA else 0), (target, aligned, valid, delta, off)
            assert got == (1 if target == 8 and aligned and valid and delta and off == 0 else 0)
            asked += got
    assert asked == 1


# ---- A2. extents and addresses beyond 2^32 ------------------------------------------------------------------------------------------------
# Targets of 2^32 + 2^24 bytes (the GPU cases of tests/test_gpu_large_outputs.py) up to 2^40 bytes (sizes no GPU test can afford), at
# bases just above 2^32, far above it, and below it with the buffer running across it.  The model is Python's integers, which do not wrap.
BIG_EXTENTS = ((1 << 32) + (1 << 24), (1 << 33) + 12345, 1 << 36, 1 << 40)
BIG_BASES = ((1 << 32) + 128, BASE, 1 << 31, (1 << 32) - 128, 0x0000300000000000 + (1 << 32))


def big_targets():
    for ts in (8, 16, 32):
        for extent in BIG_EXTENTS:
            n = -(-extent // frame(ts))
            n += (-n) % 8 + 8 * (ts != 8)              # whole units of 8 envs; at 16 / 32 one more unit
            for base in BIG_BASES:
                yield ts, n, base


def foreign_ranges(base, size, F):
    """(out, bytes) around and inside [base, base + size): just outside and one byte inside at both ends, at and around the offsets 2^31 and
    2^32, where those offsets' low 32 bits land, the last frame, everything."""
    end = base + size
    yield base - 4096, 4096
    yield base - 4096, 4097
    yield end, 4096
    yield end - 1, 4096
    yield end - 1, 1
    yield end - F, F
    yield base - 64, size + 128
    yield base + 100, 0
    for off in (1 << 31, 1 << 32, (1 << 32) + (1 << 24) - 64, size - 64):
        if 0 <= off < size:
            yield base + off, 64
    yield end + (1 << 32), 64                          # outside, at an address whose low 32 bits lie inside
    yield (base - (1 << 32) if base > (1 << 32) + 4096 else base + size + (1 << 33)), 64


def test_foreign_writes_into_targets_beyond_4_gib(lib):
    cases = 0
    for ts, n, base in big_targets():
        F = frame(ts)
        size = n * F
        assert size > (1 << 32) + (1 << 24) - F
        for out, nbytes in foreign_ranges(base, size, F):
            for entry in ("foreign", "another tile size", "listed rows"):
                lib.tg_new()
                lib.tg_register(base, ts, n)
                lib.tg_force(1, 0)
                before = state(lib)
                assert before[0] == base and before[6] == n
                if entry == "foreign":
                    kind = lib.tg_foreign(out, nbytes)
                elif entry == "another tile size":
                    kind = lib.tg_plan({8: 16, 16: 32, 32: 8}[ts], out, nbytes, 0, 1, 1, 1)
                else:
                    kind = lib.tg_plan(ts, out, nbytes, 0, 1, 1, 1)
                hit = nbytes > 0 and out < base + size and out + nbytes > base         # Python integers (an empty range overlaps nothing)
                if entry == "listed rows" and ts == 8 and out == base:
                    continue                                                            # (at 8 a range from env 0 on is on target)
                assert kind == ELSEWHERE, (ts, n, hex(base), hex(out), nbytes, entry)
                assert lib.tg_valid() == (0 if hit else 1), (ts, n, hex(base), hex(out), nbytes, entry, hit)
                if not hit:
                    assert state(lib) == before
                cases += 1
    assert cases > 3 * len(BIG_EXTENTS) * len(BIG_BASES) * 11 * 3 - 100


def test_on_target_renders_of_targets_beyond_4_gib(lib):
    for ts, n, base in big_targets():
        F = frame(ts)
        # the whole batch at the registered pointer: FILL, then DELTA
        setup_big = lambda valid: (lib.tg_new(), lib.tg_register(base, ts, n), lib.tg_force(valid, 0))
        setup_big(0)
        assert lib.tg_plan(ts, base, n * F, 0, n, 0, 1) == FILL and lib.tg_shadow_off() == 0
        lib.tg_commit(1)
        assert lib.tg_valid() == 1 and lib.tg_filled() == n
        assert lib.tg_plan(ts, base, n * F, 0, n, 0, 1) == DELTA
        if ts != 8:
            continue
        assert lib.tg_query(base, 1) == 1 and lib.tg_query(base + (1 << 32), 1) == 0
        # bbai_step_render's halves at 8: a range that starts on a unit of envs, its rows beyond 2^31 / 2^32 bytes into the buffer
        for env_off in sorted({8 * (((1 << 31) // F + 8) // 8), 8 * (((1 << 32) // F + 8) // 8), n - 8, 8 * ((n // 2) // 8)}):
            nr = n - env_off
            assert env_off % 8 == 0 and 0 < env_off < n
            setup_big(1)
            assert lib.tg_plan(8, base + env_off * F, nr * F, env_off, nr, 0, 1) == DELTA, (n, hex(base), env_off)
            assert lib.tg_shadow_off() == env_off * 49 and lib.tg_valid() == 1
            # the same rows 2^32 bytes further on or back, or one env off: not those envs' rows -- a foreign write where it lands in the buffer
            for wrong in (base + env_off * F + (1 << 32), base + env_off * F - (1 << 32), base + (env_off + 1) * F):
                setup_big(1)
                hit = wrong < base + n * F and wrong + nr * F > base
                assert lib.tg_plan(8, wrong, nr * F, env_off, nr, 0, 1) == ELSEWHERE and lib.tg_valid() == (0 if hit else 1), (n, hex(base), env_off, hex(wrong))
            # fills in order across the offset make the shadow valid
            setup_big(0)
            for off, cnt in ((0, env_off), (env_off, nr)):
                assert lib.tg_plan(8, base + off * F, cnt * F, off, cnt, 0, 1) == FILL and lib.tg_shadow_off() == off * 49
                lib.tg_commit(1)
            assert lib.tg_valid() == 1 and lib.tg_filled() == n


# ---- B. the GPU tests' call sequences -------------------------------------------------------------------------------------------------
class Handle(object):
    """The engine's calls as far as the target sees them (bbai_engine.hip: every render is plan, launch, commit; the launches succeed)."""
    def __init__(self, lib, n):
        self.lib, self.n, self.delta, self.next_ts = lib, n, 1, 8
        lib.tg_new()

    valid = property(lambda self: self.lib.tg_valid())

    def set_render_target(self, pixels):
        self.lib.tg_register(pixels, self.next_ts, self.n)

    def set_atlas(self):
        self.lib.tg_atlas_replaced(8)

    def set_view_atlas(self, ts):
        self.lib.tg_atlas_replaced(ts)

    def set_render_delta(self, v):
        self.delta = v
        self.lib.tg_invalidate()

    def render(self, out):                                   # bbai_render: the whole batch at 8
        kind = self.lib.tg_plan(8, out, self.n * frame(8), 0, self.n, 0, self.delta)
        self.lib.tg_commit(1)
        return kind

    def step_render(self, pixels):                           # bbai_step_render, unsplit: the query, then the render
        before = state(self.lib)
        dirty = self.lib.tg_query(pixels, self.delta)
        assert state(self.lib) == before
        assert (self.render(pixels) == DELTA) == bool(dirty)

    def render_view(self, ts, out, rows=None, count=None, ids=False):
        rows = self.n if rows is None else rows
        count = rows if count is None else count
        kind = self.lib.tg_plan(ts, out, count * frame(ts), 0, count, 1 if ids or count != rows or rows != self.n else 0, self.delta)
        self.lib.tg_commit(1)
        return kind


def pixel_env(lib, n, ts, pixels):
    """BatchedBabyAIEnv(pixel=True, tile_size=ts): the view atlas, the registration."""
    h = Handle(lib, n)
    if ts == 8:
        h.set_atlas()
    else:
        h.set_view_atlas(ts)
        h.next_ts = ts
    h.set_render_target(pixels)
    return h


def test_script_what_invalidates_the_shadow_and_what_does_not(lib):
    ts, n, P = 16, 9, BASE
    F = frame(ts)
    h = pixel_env(lib, n, ts, P)
    step = lambda: h.render_view(ts, P)                      # step() at 16: the encoded step, then the whole batch into self.pixels
    assert step() == FILL                                    # reset()

    def step_and_check(what):
        step()
        assert h.valid == 1, what
    step_and_check("first step")
    h.render_view(ts, FAR, count=2, ids=True)                # render_view([0, 1])
    h.set_view_atlas(32)
    h.render_view(32, FAR, count=1, ids=True)                # render_view([2], tile_size=32)
    h.set_atlas()
    h.render(FAR)                                            # render_view(tile_size=8)
    h.render_view(32, FAR, rows=2)                           # render_encoding(image[:2], tile_size=32)
    h.render_view(ts, FAR)                                   # render_encoding(out=<a buffer of its own>)
    assert h.valid == 1
    step_and_check("after renders elsewhere")
    h.render_view(ts, P + 2 * F, count=2, ids=True)
    assert h.valid == 0
    step_and_check("render_view(ids) into a slice")
    h.render_view(ts, P, rows=4)
    assert h.valid == 0
    step_and_check("a partial count")
    h.render_view(32, P, rows=2)
    assert h.valid == 0
    step_and_check("tile size 32 into the buffer")
    assert n * frame(8) + n * frame(8) <= n * F
    h.render(P + n * frame(8))
    assert h.valid == 0
    step_and_check("tile size 8 into the buffer, past n * 9408 bytes")
    lib.tg_invalidate()
    assert h.valid == 0
    step_and_check("bbai_render_invalidate")
    h.set_view_atlas(ts)
    assert h.valid == 0
    step_and_check("the view atlas installed again")
    h.set_render_delta(0)
    assert h.valid == 0
    assert step() == ELSEWHERE
    assert h.valid == 0
    h.set_render_delta(1)
    assert h.valid == 0
    step_and_check("render_delta back at 1")
    lib.tg_invalidate()
    assert h.valid == 0
    step_and_check("the caller's own write + bbai_render_invalidate")
    assert step() == DELTA and h.valid == 1


def test_script_the_tile_size_8_planner_leaves_a_16_target_alone(lib):
    n, ts, T = 16, 16, BASE
    h = Handle(lib, n)                                       # an encoded batch: nothing registered
    h.set_atlas()
    h.set_view_atlas(ts)
    h.next_ts = ts
    h.set_render_target(T)
    assert h.render_view(ts, T) == FILL
    assert h.valid == 1
    assert h.render(FAR) == ELSEWHERE
    assert h.valid == 1
    assert h.render(T) == ELSEWHERE                          # the registered buffer's first n * 9408 bytes
    assert h.valid == 0
    assert lib.tg_query(T, 1) == 0
    h.step_render(T)
    assert h.valid == 0
    assert h.render_view(ts, T) == FILL
    assert h.valid == 1


def test_script_delta_history_events(lib):
    n, P = 4096 + 8 + 1, BASE
    h = pixel_env(lib, n, 8, P)
    assert h.render(P) == FILL                               # reset()

    def run(k):
        for _ in range(k):
            h.step_render(P)
    run(20)
    assert h.valid == 1
    lib.tg_invalidate()
    assert h.valid == 0
    run(10)
    assert h.render(FAR) == ELSEWHERE                        # render_encoding(out=other)
    assert h.valid == 1
    run(10)
    h.set_atlas()
    assert h.valid == 0
    run(10)
    assert h.valid == 1
    h.set_atlas()
    run(10)
    h.set_render_delta(0)
    run(3)
    assert h.valid == 0
    h.set_render_delta(1)
    run(10)
    assert h.valid == 1


@pytest.mark.parametrize("offset", [0, 16])
def test_script_delta_registered_buffer_alignment(lib, offset):
    n = 131072 + 5
    own, buf = FAR, BASE + offset                            # a.pixels, and the test's buffer 0 / 16 bytes off the 128-byte grid
    h = pixel_env(lib, n, 8, own)
    assert h.render(own) == FILL
    h.set_render_target(buf)
    for t in range(40):
        h.step_render(own)                                   # no longer the target: full renders
        kind = h.render(buf)
        assert kind == (ELSEWHERE if offset else FILL if t == 0 else DELTA)
    assert h.valid == (1 if offset == 0 else 0)
