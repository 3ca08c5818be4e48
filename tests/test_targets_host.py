"""The handle's two registered targets side by side (babyai_amd/csrc/bbai_target.hpp: Targets, the three plan_target entries, commit_target)
without a GPU: the header compiled with g++ from a wrapper this test writes, both targets registered at made-up addresses -- disjoint,
adjacent, one inside the other, at the same base; small, and with bases and extents across 2^32 and 2^33 -- and driven through the three
entries.  The model is Python's integers: an entry invalidates exactly the targets its bytes intersect, an on-target plan leaves its own
target's state to the commit, a failed commit invalidates only what the plan covered; and the grid target's commit is what it was as a
record of its own, `valid = ok`."""
import ctypes
import os
import subprocess

import pytest

from test_render_target_host import BASE, BIG_BASES, foreign_ranges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "babyai_amd", "csrc")
ELSEWHERE, FILL, DELTA = 0, 1, 2
VIEW, GRID = 0, 1
FV = 147 * 8 * 8                    # a view frame at tile size 8: 9408 bytes (8 of them: 588 lines of 128 bytes)

WRAPPER = """
#include "bbai_target.hpp"
using namespace bbai;
static Targets g;
static TargetPlan g_plan;
static Target& pick(int which) { return which ? g.grid : static_cast<Target&>(g.view); }
static int kind() { return g_plan.kind == TargetPlan::ELSEWHERE ? 0 : g_plan.kind == TargetPlan::FILL ? 1 : 2; }
extern "C" {
void tt_new() { g = Targets(); }
void tt_register(int which, unsigned long long pixels, int ts, long long n, long long frame_bytes) {
    pick(which).shadow = reinterpret_cast<uint8_t*>(uintptr_t(1) << (20 + which));          // (an address nobody reads)
    register_target(pick(which), (uintptr_t)pixels, ts, n, frame_bytes);
}
void tt_force(int which, int valid, long long filled) { pick(which).valid = valid != 0; pick(which).filled = filled; }
int tt_plan_view(int ts, unsigned long long out, long long bytes, long long env_off, long long nr, int partial, int delta) {
    g_plan = plan_target(g, RenderRequest{ts, (uintptr_t)out, bytes, env_off, nr, partial != 0, delta != 0});
    return kind();
}
int tt_plan_grid(int delta) { g_plan = plan_target(g, GridRenderRequest{delta != 0}); return kind(); }
int tt_plan_write(unsigned long long out, long long bytes) { g_plan = plan_target(g, WriteRequest{(uintptr_t)out, bytes}); return kind(); }
int tt_plan_covers_grid() { return g_plan.grid ? 1 : 0; }
void tt_commit(int ok) { commit_target(g, g_plan, ok != 0); }
void tt_state(int which, unsigned long long* s) {
    const Target& t = pick(which);
    s[0] = t.pixels; s[1] = (unsigned long long)t.ts; s[2] = (uintptr_t)t.shadow; s[3] = t.valid; s[4] = (unsigned long long)t.filled;
    s[5] = (unsigned long long)t.n; s[6] = (unsigned long long)t.frame_bytes;
}
long long tt_frame_bytes(int which, long long cells, int ts) { return which ? grid_frame_bytes(cells, ts) : view_frame_bytes(ts); }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("targets_host")
    src, so = str(d / "wrapper.cpp"), str(d / "libtargets.so")
    with open(src, "w") as f:
        f.write(WRAPPER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-I", CSRC, "-o", so, src])
    lib = ctypes.CDLL(so)
    U, L, I = ctypes.c_ulonglong, ctypes.c_longlong, ctypes.c_int
    for name, res, args in (("tt_new", None, []), ("tt_register", None, [I, U, I, L, L]), ("tt_force", None, [I, I, L]),
                            ("tt_plan_view", I, [I, U, L, L, L, I, I]), ("tt_plan_grid", I, [I]), ("tt_plan_write", I, [U, L]),
                            ("tt_plan_covers_grid", I, []), ("tt_commit", None, [I]), ("tt_state", None, [I, ctypes.POINTER(U)]),
                            ("tt_frame_bytes", L, [I, L, I])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def state(lib, which):
    s = (ctypes.c_ulonglong * 7)()
    lib.tt_state(which, s)
    return tuple(s)


def valid(lib, which):
    return state(lib, which)[3]


def invalid_state(before):
    return before[:3] + (0, 0) + before[5:]


class Layout(object):
    """Two registered targets: the view's at tile size 8 (nv envs), the grid's W x H at tile size 8 (ng envs: the record asks no more of
    a batch than its own count)."""
    def __init__(self, name, vb, nv, gb, ng, cells):
        self.name, self.vb, self.nv, self.gb, self.ng, self.cells = name, vb, nv, gb, ng, cells
        self.FG = 3 * cells * 64
        self.VS, self.GS = nv * FV, ng * self.FG

    def register(self, lib, view_valid, grid_valid):
        lib.tt_new()
        assert lib.tt_frame_bytes(VIEW, 0, 8) == FV and lib.tt_frame_bytes(GRID, self.cells, 8) == self.FG
        lib.tt_register(VIEW, self.vb, 8, self.nv, FV)
        lib.tt_register(GRID, self.gb, 8, self.ng, self.FG)
        assert valid(lib, VIEW) == 0 and valid(lib, GRID) == 0                 # a history starts invalid
        lib.tt_force(VIEW, view_valid, self.nv if view_valid else 0)
        lib.tt_force(GRID, grid_valid, self.ng if grid_valid else 0)
        return state(lib, VIEW), state(lib, GRID)

    def hits(self, out, nbytes):                                               # Python integers, which do not wrap
        return (nbytes > 0 and out < self.vb + self.VS and out + nbytes > self.vb,
                nbytes > 0 and out < self.gb + self.GS and out + nbytes > self.gb)

    def __repr__(self):
        return "%s: view %#x + %d, grid %#x + %d" % (self.name, self.vb, self.VS, self.gb, self.GS)


def down128(x):
    return x // 128 * 128


def layouts_at(B, nv, ng, cells):
    VS, GS = nv * FV, ng * 3 * cells * 64
    assert B % 128 == 0 and VS % 128 == 0 and GS % 128 == 0                    # every base below: on a 128-byte line
    yield Layout("disjoint", B, nv, B + VS + 4096, ng, cells)
    yield Layout("disjoint, the grid first", B + GS + 4096, nv, B, ng, cells)
    yield Layout("adjacent", B, nv, B + VS, ng, cells)
    yield Layout("adjacent, the grid first", B + GS, nv, B, ng, cells)
    yield Layout("the same base", B, nv, B, ng, cells)
    if GS < VS:
        yield Layout("the grid inside the view", B, nv, B + down128((VS - GS) // 2), ng, cells)
        yield Layout("the grid at the view's end", B, nv, B + VS - GS, ng, cells)
    else:
        yield Layout("the view inside the grid", B + down128((GS - VS) // 2), nv, B, ng, cells)
        yield Layout("the view at the grid's end", B + GS - VS, nv, B, ng, cells)


def units(extent, frame):
    """Envs, in whole units of 8, whose frames cover `extent` bytes."""
    n = -(-extent // frame)
    return n + (-n) % 8


def all_layouts():
    for ng, cells in ((8, 16), (8, 22 * 22)):                                  # the grid smaller than the view (8 x 9408 B), and larger
        for lay in layouts_at(BASE, 8, ng, cells):
            yield lay
    big = ((1 << 32) + (1 << 24), (1 << 33) + 12345)
    for ve, ge in ((big[0], big[1]), (big[1], big[0]), (big[1], 1 << 20)):     # each of the two across 2^32 / 2^33, and a small grid in a large view
        for B in BIG_BASES:
            for lay in layouts_at(B, units(ve, FV), units(ge, 3 * 16 * 64), 16):
                yield lay


def ranges_of(lay):
    seen = set()
    for base, size, F in ((lay.vb, lay.VS, FV), (lay.gb, lay.GS, lay.FG)):
        for r in foreign_ranges(base, size, F):
            if r not in seen:
                seen.add(r)
                yield r


def expect_after_foreign(lib, lay, before, hit, own=None):
    """Each target: untouched where the bytes miss it (or where it is the plan's own), history gone where they hit."""
    for which in (VIEW, GRID):
        if which == own or not hit[which]:
            assert state(lib, which) == before[which], (lay, which)
        else:
            assert state(lib, which) == invalid_state(before[which]), (lay, which)


def test_any_other_write_tells_both(lib):
    cases, both, one = 0, 0, 0
    for lay in all_layouts():
        for out, nbytes in ranges_of(lay):
            hit = lay.hits(out, nbytes)
            for ok in (1, 0):
                before = lay.register(lib, 1, 1)
                assert lib.tt_plan_write(out, nbytes) == ELSEWHERE, (lay, hex(out), nbytes)
                expect_after_foreign(lib, lay, before, hit)
                planned = state(lib, VIEW), state(lib, GRID)
                lib.tt_commit(ok)                                              # nothing covered: nothing to settle, whatever the outcome
                assert (state(lib, VIEW), state(lib, GRID)) == planned, (lay, hex(out), nbytes, ok)
            cases += 1
            both += hit[0] and hit[1]
            one += hit[0] != hit[1]
    assert cases > 2 * 7 * 14 + 3 * len(BIG_BASES) * 7 * 14 and both > 100 and one > 100


def test_a_view_render_plans_the_view_target_and_tells_the_grid_target(lib):
    for lay in all_layouts():
        hit = lay.hits(lay.vb, lay.VS)
        assert hit[VIEW]
        for view_valid in (1, 0):
            for ok in (1, 0):
                before = lay.register(lib, view_valid, 1)
                kind = lib.tt_plan_view(8, lay.vb, lay.VS, 0, lay.nv, 0, 1)
                assert kind == (DELTA if view_valid else FILL) and lib.tt_plan_covers_grid() == 0, lay
                expect_after_foreign(lib, lay, before, hit, own=VIEW)          # its own target's state: left to the commit
                grid_planned = state(lib, GRID)
                lib.tt_commit(ok)
                assert state(lib, GRID) == grid_planned, lay                   # a commit settles only what the plan covered
                if ok:
                    assert state(lib, VIEW) == before[VIEW][:3] + (1, lay.nv) + before[VIEW][5:], lay
                else:
                    assert state(lib, VIEW) == invalid_state(before[VIEW]), lay
        # a render that is not one of target envs into their rows -- another tile size, "render_delta" 0, a listed row: a write like any other
        for out, nbytes in ranges_of(lay):
            hit = lay.hits(out, nbytes)
            for ts, partial, delta in ((16, 0, 1), (8, 0, 0), (32, 1, 1)):
                before = lay.register(lib, 1, 1)
                assert lib.tt_plan_view(ts, out, nbytes, 0, 1, partial, delta) == ELSEWHERE, (lay, hex(out), nbytes, ts)
                expect_after_foreign(lib, lay, before, hit)
                planned = state(lib, VIEW), state(lib, GRID)
                lib.tt_commit(0)
                assert (state(lib, VIEW), state(lib, GRID)) == planned, (lay, hex(out), nbytes, ts)


def test_a_grid_render_plans_the_grid_target_and_tells_the_view_target(lib):
    for lay in all_layouts():
        hit = lay.hits(lay.gb, lay.GS)
        assert hit[GRID]
        for grid_valid in (1, 0):
            for delta in (1, 0):
                for ok in (1, 0):
                    before = lay.register(lib, 1, grid_valid)
                    kind = lib.tt_plan_grid(delta)
                    # with the option off still an on-target FILL: whole frames, every tile id behind them
                    assert kind == (DELTA if grid_valid and delta else FILL) and lib.tt_plan_covers_grid() == 1, lay
                    expect_after_foreign(lib, lay, before, hit, own=GRID)
                    view_planned = state(lib, VIEW)
                    lib.tt_commit(ok)
                    assert state(lib, VIEW) == view_planned, lay
                    # the grid target's commit as a record of its own was `valid = ok`, for FILL and DELTA alike
                    assert valid(lib, GRID) == ok, (lay, grid_valid, delta, ok)
                    if ok:
                        assert state(lib, GRID) == before[GRID][:3] + (1, lay.ng) + before[GRID][5:], lay
                    else:
                        assert state(lib, GRID) == invalid_state(before[GRID]), lay


def test_an_unregistered_target_is_never_told(lib):
    lay = next(layouts_at(BASE, 8, 8, 16))
    for gone in (VIEW, GRID):
        before = lay.register(lib, 1, 1)
        lib.tt_register(gone, 0, 8, 8, before[gone][6])
        cleared = state(lib, gone)
        assert cleared[0] == 0 and cleared[3] == 0 and cleared[2] == before[gone][2]          # no history; the shadow stays
        base, size = (lay.vb, lay.VS) if gone == VIEW else (lay.gb, lay.GS)
        assert lib.tt_plan_write(base, size) == ELSEWHERE and state(lib, gone) == cleared
        assert state(lib, 1 - gone) == before[1 - gone]                        # (disjoint: the other one's bytes were not written)
        if gone == VIEW:
            assert lib.tt_plan_view(8, base, size, 0, 8, 0, 1) == ELSEWHERE
        else:
            assert lib.tt_plan_grid(1) == ELSEWHERE
        lib.tt_commit(1)
        assert state(lib, gone) == cleared and state(lib, 1 - gone) == before[1 - gone]
