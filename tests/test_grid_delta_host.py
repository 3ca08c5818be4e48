"""The registered full-grid target on the host (include/bbai_grid_target.h; babyai_amd/csrc/bbai_gridtarget.hpp and bbai_target.hpp, compiled here with g++):
the geometry of a frame's 64-byte pieces against grid_delta_util's, which is written from the picture alone; the planner's state machine
with made-up addresses; and the C ABI of the five entries against engine.ABI_GRID_TARGET.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import grid_delta_util as gdu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bbai_grid_target.h")
NAMES = ("bbai_set_grid_target", "bbai_render_grid_target", "bbai_step_grid_target", "bbai_grid_target_invalidate", "bbai_grid_target_shadow")
GRIDS = sorted(gdu.level_grids())

_SRC = r"""
#include "bbai_gridtarget.hpp"
#include "bbai_target.hpp"
using namespace bbai;
extern "C" int gd_ok(int W, int H, int ts) { return grid_geom_ok(W, H, ts) ? 1 : 0; }
extern "C" uint32_t gd_pieces(int W, int H, int ts) { return grid_geom(W, H, ts).NP; }
extern "C" void gd_segments(int W, int H, int ts, int* n, int* y0, uint32_t* c0, int* y1, uint32_t* c1) {
    const GridGeom g = grid_geom(W, H, ts);
    for (uint32_t p = 0; p < g.NP; ++p) {
        const GridSegs s = grid_piece_segments(g, p);
        const GridSegs t = grid_piece_segments(W, ts, p);       // the (W, ts, p) form: the same
        n[p] = s.n == t.n && s.s[0].y == t.s[0].y && s.s[0].cols == t.s[0].cols && s.s[1].cols == t.s[1].cols ? s.n : -1;
        y0[p] = s.s[0].y; c0[p] = s.s[0].cols;
        y1[p] = s.n > 1 ? s.s[1].y : -1; c1[p] = s.n > 1 ? s.s[1].cols : 0;
    }
}
// the pieces a set of changed cells marks: every piece judged (all[p]), and the kernel's walk -- only the tile rows whose mask is
// non-zero, each row its own pieces [grid_row_first(y), grid_row_first(y + 1)) -- with how often each piece was judged
extern "C" void gd_dirty(int W, int H, int ts, const uint32_t* rows /* [H + 1], the last one 0 */, uint8_t* all, uint8_t* walked, uint8_t* judged) {
    const GridGeom g = grid_geom(W, H, ts);
    for (uint32_t p = 0; p < g.NP; ++p) all[p] = grid_piece_dirty(g, p, rows) ? 1 : 0;
    for (int y = 0; y < H; ++y) {
        if (!rows[y]) continue;
        for (uint32_t p = grid_row_first(g, y); p < grid_row_first(g, y + 1); ++p) { judged[p]++; if (grid_piece_dirty(g, p, rows)) walked[p] = 1; }
    }
}
extern "C" void gd_row_first(int W, int H, int ts, uint32_t* first /* [H + 1] */) {
    const GridGeom g = grid_geom(W, H, ts);
    for (int y = 0; y <= H; ++y) first[y] = grid_row_first(g, y);
}
// k_grid_delta's launch shape
extern "C" int gd_group(int W, int H, int ES) { return griddelta_group(W, H, ES); }
extern "C" void gd_shape(int64_t n, int64_t blocks, int W, int H, int ES, int asked, int64_t* out) {
    const GridDeltaShape s = griddelta_shape(n, blocks, W, H, ES, asked);
    out[0] = s.envs_per_group; out[1] = s.groups;
}
extern "C" void gd_shape_constants(int* c) {
    c[0] = GRIDDELTA_BLOCK; c[1] = GRIDDELTA_MAX_ENVS; c[2] = GRIDDELTA_APP; c[3] = GRIDDELTA_IDS; c[4] = GRIDDELTA_BPC; c[5] = MAX_W;
}
// the planner, on one record
static Targets BOTH;                      // (the view target stays un-registered)
static GridTarget& T = BOTH.grid;
static uint8_t SHADOW[4];
extern "C" void gt_register(uint64_t pixels, int ts, int64_t n, int64_t cells) { if (pixels) T.shadow = SHADOW; register_target(T, (uintptr_t)pixels, ts, n, grid_frame_bytes(cells, ts)); }
extern "C" int gt_render(int delta, int ok) { const TargetPlan p = plan_target(BOTH, GridRenderRequest{delta != 0}); const int k = (int)p.kind; commit_target(BOTH, p, ok != 0); return k; }
extern "C" int gt_plan(int delta) { return (int)plan_target(BOTH, GridRenderRequest{delta != 0}).kind; }
extern "C" int gt_foreign(uint64_t out, int64_t bytes) { const bool hit = overlaps_target(T, (uintptr_t)out, bytes); (void)plan_target(BOTH, WriteRequest{(uintptr_t)out, bytes}); return hit ? 1 : 0; }
extern "C" void gt_atlas(int ts) { target_atlas_replaced(T, ts); }
extern "C" void gt_invalidate() { invalidate_target(T); }
extern "C" int gt_valid() { return T.valid ? 1 : 0; }
extern "C" uint64_t gt_pixels() { return (uint64_t)T.pixels; }
extern "C" int64_t gt_bytes() { return target_bytes(T); }
extern "C" int gt_has_shadow() { return T.shadow ? 1 : 0; }
extern "C" int gt_constants(int k) { return k == 0 ? GRID_PIECE : k == 1 ? GRID_TARGET_ALIGN : (int)TargetPlan::FILL * 10 + (int)TargetPlan::DELTA; }
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("grid_delta")
    src, so = str(d / "grid_delta.cpp"), str(d / "libgrid_delta.so")
    with open(src, "w") as f:
        f.write(_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-I" + os.path.join(ROOT, "babyai_amd", "csrc"), "-o", so, src])
    L = ctypes.CDLL(so)
    P, I, I64, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
    L.gd_ok.argtypes = [I, I, I]
    L.gd_pieces.argtypes, L.gd_pieces.restype = [I, I, I], ctypes.c_uint32
    L.gd_segments.argtypes, L.gd_segments.restype = [I, I, I, P, P, P, P, P], None
    L.gd_dirty.argtypes, L.gd_dirty.restype = [I, I, I, P, P, P, P], None
    L.gd_row_first.argtypes, L.gd_row_first.restype = [I, I, I, P], None
    L.gd_group.argtypes = [I, I, I]
    L.gd_shape.argtypes, L.gd_shape.restype = [I64, I64, I, I, I, I, P], None
    L.gd_shape_constants.argtypes, L.gd_shape_constants.restype = [P], None
    L.gt_register.argtypes, L.gt_register.restype = [U64, I, I64, I64], None
    L.gt_render.argtypes = [I, I]
    L.gt_plan.argtypes = [I]
    L.gt_foreign.argtypes = [U64, I64]
    L.gt_atlas.argtypes, L.gt_atlas.restype = [I], None
    L.gt_invalidate.restype = None
    L.gt_pixels.restype = U64
    L.gt_bytes.restype = I64
    L.gt_constants.argtypes = [I]
    return L


# ---- the geometry -------------------------------------------------------------------------------------------------------------------
def test_the_levels_grids():
    assert len(GRIDS) >= 20 and {(4, 4), (7, 3), (8, 8), (22, 22)} <= set(GRIDS)


@pytest.mark.parametrize("ts", gdu.TILE_SIZES)
def test_every_piece_of_every_grid_has_the_geometrys_segments(lib, ts):
    assert lib.gt_constants(0) == gdu.PIECE == 64 and lib.gt_constants(1) == 64
    straddle = {}
    for W, H in GRIDS:
        assert lib.gd_ok(W, H, ts) == 1
        F = gdu.frame_bytes(W, H, ts)
        assert F % 64 == 0 and lib.gd_pieces(W, H, ts) == F // 64
        n, y0, c0, y1, c1 = gdu.piece_segments(W, H, ts)
        got = [np.zeros(F // 64, np.int32), np.zeros(F // 64, np.int32), np.zeros(F // 64, np.uint32), np.zeros(F // 64, np.int32), np.zeros(F // 64, np.uint32)]
        lib.gd_segments(W, H, ts, *[a.ctypes.data for a in got])
        for name, g, w in zip(("n", "y0", "cols0", "y1", "cols1"), got, (n, y0, c0, y1, c1)):
            bad = np.nonzero(g.astype(np.int64) != np.asarray(w, np.int64))[0]
            assert len(bad) == 0, (W, H, ts, name, bad[:4].tolist())
        assert n.max() == 1                    # a tile row is 3 W ts^2 bytes, a whole number of pieces: no piece lies in two tile rows
        rb = 3 * W * ts
        straddle[(W, H)] = int(((np.arange(F // 64) * 64) // rb != (np.arange(F // 64) * 64 + 63) // rb).sum())      # ... but in two PIXEL rows
        # [first(y), first(y + 1)) partitions the frame into the tile rows' pieces
        first = np.zeros(H + 1, np.uint32)
        lib.gd_row_first(W, H, ts, first.ctypes.data)
        start_row = (np.arange(F // 64, dtype=np.int64) * 64 // (3 * W * ts)) // ts
        assert first[0] == 0 and first[H] == F // 64
        for y in range(H):
            assert (start_row[first[y]:first[y + 1]] == y).all() and (first[y] == 0 or start_row[first[y] - 1] < y), (W, H, ts, y)
        assert (y0 == start_row).all()
    # 96-, 168- and 528-byte pixel rows (W = 4, 7, 22 at 8): pieces span two pixel rows; rows of a multiple of 64 bytes (W = 8, 16): never
    assert straddle[(8, 8)] == 0 and straddle[(16, 16)] == 0
    if ts == 8:
        assert straddle[(4, 4)] > 0 and straddle[(22, 22)] > 0 and straddle[(7, 3)] > 0
    assert lib.gd_ok(2, 4, ts) == 0 and lib.gd_ok(26, 4, ts) == 0 and lib.gd_ok(8, 8, 12) == 0


def _marks(lib, W, H, ts, changed):
    """(all, walked, judged) of the header for bool[H, W] changed cells."""
    rows = np.zeros(H + 1, np.uint32)
    for y in range(H):
        rows[y] = sum(1 << x for x in range(W) if changed[y, x])
    npieces = gdu.frame_bytes(W, H, ts) // 64
    out = [np.zeros(npieces, np.uint8) for _ in range(3)]
    lib.gd_dirty(W, H, ts, rows.ctypes.data, *[a.ctypes.data for a in out])
    return out


def _dirty_sets(W, H, rng):
    sets = [np.zeros((H, W), bool), np.ones((H, W), bool)]
    for _ in range(3):
        y, x = rng.randint(0, H), rng.randint(0, W)
        one = np.zeros((H, W), bool)
        one[y, x] = True
        sets.append(one)
        hor = one.copy()
        hor[y, x + 1 if x + 1 < W else x - 1] = True
        sets.append(hor)
        ver = one.copy()
        ver[y + 1 if y + 1 < H else y - 1, x] = True
        sets.append(ver)
    for corner in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        c = np.zeros((H, W), bool)
        c[corner] = True
        sets.append(c)
    for dens in (0.02, 0.1, 0.5):
        sets.append(rng.rand(H, W) < dens)
    return sets


@pytest.mark.parametrize("ts", gdu.TILE_SIZES)
def test_marked_pieces_are_stored_mask(lib, ts):
    rng = np.random.RandomState(ts)
    for W, H in GRIDS:
        if ts == 32 and W * H > 64 and (W, H) != (22, 22):
            continue                                       # (the large frames at 32: BossLevel's stands for them)
        before = rng.randint(0, 100, size=(1, H * W)).astype(np.uint8)
        for changed in _dirty_sets(W, H, rng):
            after = np.where(changed.reshape(1, -1), before + 1, before).astype(np.uint8)
            want = gdu.stored_mask(before, after, W, H, ts)[0]
            every, walked, judged = _marks(lib, W, H, ts, changed)
            assert np.array_equal(every.astype(bool), want), (W, H, ts, np.argwhere(changed)[:4].tolist())
            assert np.array_equal(walked.astype(bool), want), (W, H, ts, "the rows' walk misses or adds a piece")
            assert judged.max(initial=0) <= 1                  # every piece judged once at most
            assert want.any() == changed.any()
            if changed.all():
                assert want.all() and (judged == 1).all()


def test_stored_mask_of_a_known_case():
    """4 x 4 at tile size 8: 96-byte pixel rows.  Cell (x = 0, y = 1) is bytes [0, 24) of pixel rows 8 .. 15: 768 + 96 k + [0, 24)."""
    before = np.zeros((1, 16), np.uint8)
    after = before.copy()
    after[0, 1 * 4 + 0] = 1
    want = sorted({(768 + 96 * k + b) // 64 for k in range(8) for b in range(24)})
    assert np.nonzero(gdu.stored_mask(before, after, 4, 4, 8)[0])[0].tolist() == want == [12, 13, 15, 16, 18, 19, 21, 22]
    n, y0, c0, y1, c1 = gdu.piece_segments(4, 4, 8)
    assert (n[11], y0[11], c0[11], y1[11]) == (1, 0, 0b1110, -1)           # bytes [704, 768): [32, 96) of pixel row 7, all of tile row 0
    assert (n[12], y0[12], c0[12]) == (1, 1, 0b0111)                         # bytes [768, 832) of pixel row 8: columns 0 .. 2
    assert (n[13], y0[13], c0[13]) == (1, 1, 0b1111)                         # [64, 96) of pixel row 8 (columns 2, 3) and [0, 32) of row 9 (0, 1): one tile row, one segment


# ---- the launch shape ---------------------------------------------------------------------------------------------------------------
def test_a_group_fits_the_kernels_planes_on_every_levels_grid(lib):
    """griddelta_group / griddelta_shape for the grid and record rows of all 105 levels: a group's cells fit the id plane, its record rows
    the row plane, its listed rows the row list (entry = env * 32 + y), and it is the largest such group; the option is clamped to it."""
    from babyai_amd import levels
    c = np.zeros(6, np.int32)
    lib.gd_shape_constants(c.ctypes.data)
    block, max_envs, app, ids, bpc, max_w = (int(v) for v in c)
    assert (block, max_envs, bpc) == (512, 32, 2) and app == 4 * block and ids == 8 * block
    out = np.zeros(2, np.int64)
    seen = {}
    for name in levels.LEVELS:
        cfg = levels.make_cfg("BabyAI-%s-v0" % name)
        W, H, ES = int(cfg.W), int(cfg.H), int(cfg.ES)
        assert ES % 4 == 0 and W <= max_w and H <= max_w < 32
        G = lib.gd_group(W, H, ES)
        rd = H * ES // 4
        assert 1 <= G <= max_envs and G * W * H <= ids and G * rd <= app and G * H <= max_envs * max_w, (name, G)
        assert G == max_envs or (G + 1) * W * H > ids or (G + 1) * rd > app, (name, G)
        seen[name] = G
        blocks = 256 * bpc
        for n in (1, 3, 130, blocks - 1, blocks, 2 * blocks + 3, G * blocks - 1, G * blocks, G * blocks + 13, 1 << 20):
            for asked in (0, 1, 5, 8, 32, 1000):
                lib.gd_shape(n, blocks, W, H, ES, asked, out.ctypes.data)
                g, groups = int(out[0]), int(out[1])
                want = min(G, asked) if asked else max(1, min(G, n // blocks))
                assert g == want and groups == -(-n // g) and (groups - 1) * g < n <= groups * g, (name, n, asked, g, groups)
    assert seen["BossLevel"] == 8 and seen["GoToLocal"] == 32 and seen["GoToObjS4"] == 32


# ---- the planner --------------------------------------------------------------------------------------------------------------------
def test_planner_state_machine(lib):
    FILL, DELTA = divmod(lib.gt_constants(2), 10)
    base, n, cells, ts = 1 << 20, 10, 16, 8
    nbytes = n * 3 * cells * ts * ts
    assert lib.gt_valid() == 0 and lib.gt_pixels() == 0
    assert lib.gt_foreign(base, 64) == 0                       # nothing registered: nothing overlaps
    lib.gt_register(base, ts, n, cells)
    assert lib.gt_valid() == 0 and lib.gt_pixels() == base and lib.gt_bytes() == nbytes and lib.gt_has_shadow() == 1
    assert lib.gt_plan(1) == FILL and lib.gt_valid() == 0      # a plan alone changes nothing
    assert lib.gt_render(1, 1) == FILL and lib.gt_valid() == 1
    assert lib.gt_render(1, 1) == DELTA and lib.gt_valid() == 1
    assert lib.gt_render(0, 1) == FILL and lib.gt_valid() == 1             # option off: whole frames, the shadow kept
    # foreign ranges: just outside on both sides, then overlapping by one byte on each side, then inside, then covering
    assert lib.gt_foreign(base - 4096, 4096) == 0 and lib.gt_valid() == 1          # ends exactly where the buffer starts
    assert lib.gt_foreign(base + nbytes, 4096) == 0 and lib.gt_valid() == 1        # starts exactly where it ends
    assert lib.gt_foreign(base + 100, 0) == 0 and lib.gt_valid() == 1              # an empty write
    for out, size in ((base - 4096, 4097), (base + nbytes - 1, 4096), (base + 640, 64), (base - 64, nbytes + 128)):
        assert lib.gt_render(1, 1) in (FILL, DELTA) and lib.gt_valid() == 1
        assert lib.gt_foreign(out, size) == 1 and lib.gt_valid() == 0, (out, size)
        assert lib.gt_plan(1) == FILL
    # the atlas
    lib.gt_render(1, 1)
    lib.gt_atlas(16)
    lib.gt_atlas(32)
    assert lib.gt_valid() == 1
    lib.gt_atlas(8)
    assert lib.gt_valid() == 0
    # a failed commit, of either kind
    assert lib.gt_render(1, 0) == FILL and lib.gt_valid() == 0
    lib.gt_render(1, 1)
    assert lib.gt_render(1, 0) == DELTA and lib.gt_valid() == 0
    # explicit invalidation, re-registration
    lib.gt_render(1, 1)
    lib.gt_invalidate()
    assert lib.gt_valid() == 0
    lib.gt_render(1, 1)
    lib.gt_register(base, ts, n, cells)
    assert lib.gt_valid() == 0
    lib.gt_render(1, 1)
    lib.gt_register(base + 64, 32, n, cells)
    assert lib.gt_valid() == 0 and lib.gt_bytes() == 16 * nbytes
    # un-register: no history, nothing overlaps, the shadow stays
    lib.gt_render(1, 1)
    lib.gt_register(0, 8, n, cells)
    assert lib.gt_valid() == 0 and lib.gt_pixels() == 0 and lib.gt_has_shadow() == 1
    assert lib.gt_foreign(base, nbytes) == 0


def test_planner_with_extents_and_addresses_beyond_4_gib(lib):
    """Targets of 2^32 + 2^24 bytes (tests/test_gpu_large_outputs.py's) up to 2^40 bytes, at bases just above 2^32, far above it and below
    it with the buffer running across it: target_bytes and the overlap test against Python's integers, which do not wrap."""
    FILL, DELTA = divmod(lib.gt_constants(2), 10)
    cases = 0
    for (W, H), ts in [((22, 22), 32), ((22, 22), 8), ((8, 8), 16), ((4, 4), 8), ((25, 25), 32)]:
        cells, F = W * H, gdu.frame_bytes(W, H, ts)
        for extent in ((1 << 32) + (1 << 24), (1 << 33) + 12345, 1 << 36, 1 << 40):
            n = -(-extent // F) + 3
            size = n * F
            for base in ((1 << 32) + 64, 0x7F0000000000, 1 << 31, (1 << 32) - 64, 0x300000000000 + (1 << 32)):
                lib.gt_register(0, 8, 0, 0)
                lib.gt_register(base, ts, n, cells)
                assert lib.gt_pixels() == base and lib.gt_bytes() == size and size > (1 << 32) + (1 << 24)
                end = base + size
                ranges = [(base - 4096, 4096), (base - 4096, 4097), (end, 4096), (end - 1, 4096), (end - 1, 1), (end - F, F), (base - 64, size + 128),
                          (base + 100, 0), (end + (1 << 32), 64), (base + size + (1 << 33), 64)]
                ranges += [(base + off, 64) for off in (1 << 31, 1 << 32, (1 << 32) + (1 << 24) - 64, size - 64)]
                if base > (1 << 32) + 4096:
                    ranges.append((base - (1 << 32), 64))
                for out, nbytes in ranges:
                    assert lib.gt_render(1, 1) in (FILL, DELTA) and lib.gt_valid() == 1
                    hit = nbytes > 0 and out < base + size and out + nbytes > base              # Python integers
                    assert lib.gt_foreign(out, nbytes) == (1 if hit else 0), (W, H, ts, n, hex(base), hex(out), nbytes)
                    assert lib.gt_valid() == (0 if hit else 1), (W, H, ts, n, hex(base), hex(out), nbytes)
                    cases += 1
    lib.gt_register(0, 8, 0, 0)
    assert cases >= 5 * 4 * 5 * 14


def test_launch_shape_at_four_million_envs(lib):
    """griddelta_shape at 2^22 + 3 envs and beyond 2^32: the groups cover the batch, the last one partial."""
    from babyai_amd import levels
    out = np.zeros(2, np.int64)
    for name in ("BossLevel", "GoToLocal", "GoToObjS4", "KeyCorridorS3R1"):
        cfg = levels.make_cfg("BabyAI-%s-v0" % name)
        W, H, ES = int(cfg.W), int(cfg.H), int(cfg.ES)
        G = lib.gd_group(W, H, ES)
        for n in ((1 << 22) + 3, (1 << 31) + 5, (1 << 32) + 3, (1 << 40) + 1):
            for blocks in (512, 608):
                for asked in (0, 1, 5, 8, 32):
                    lib.gd_shape(n, blocks, W, H, ES, asked, out.ctypes.data)
                    g, groups = int(out[0]), int(out[1])
                    want = min(G, asked) if asked else max(1, min(G, n // blocks))
                    assert g == want and groups == -(-n // g) and (groups - 1) * g < n <= groups * g, (name, n, blocks, asked, g, groups)
                    assert n % g != 0 or g == 1, (name, n, g)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def prototypes():
    """{entry: [kind of every parameter]} of include/bbai_grid_target.h; kinds "ptr", "i64", "int"."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(bbai_[a-z_]+)\s*\(([^)]*)\)\s*;", text):
        assert ret.strip() == "int" and name not in out, name
        kinds = []
        for p in params.split(","):
            words = [w for w in p.split() if w != "const"]
            kinds.append("ptr" if "*" in p else {"int64_t": "i64", "int": "int"}[words[0]])
        out[name] = kinds
    return out


def test_every_prototype_has_its_table_row():
    from babyai_amd import engine
    protos = prototypes()
    assert list(protos) == list(NAMES) == list(engine.ABI_GRID_TARGET)
    assert engine.GRID_TARGET_SYMBOLS == tuple(engine.ABI_GRID_TARGET)
    assert not set(engine.ABI_GRID_TARGET) & (set(engine.ABI) | set(engine.ABI_REPLAY) | set(engine.ABI_VIEW) | set(engine.ABI_VIEW_PIXELS))
    kind = {ctypes.c_void_p: "ptr", ctypes.c_int64: "i64", ctypes.c_int: "int"}
    for name, params in protos.items():
        restype, argtypes = engine.ABI_GRID_TARGET[name]
        assert restype is ctypes.c_int and [kind[t] for t in argtypes] == params, name
    # the stepping entry takes exactly what bbai_step takes; the shadow entry what bbai_render_shadow takes
    assert engine.ABI_GRID_TARGET["bbai_step_grid_target"] == engine.ABI["bbai_step"]
    assert engine.ABI_GRID_TARGET["bbai_grid_target_shadow"] == engine.ABI["bbai_render_shadow"]
    subprocess.check_call(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", HEADER])
    text = open(HEADER).read()
    for word in ("RGBImgObsWrapper", "oracle/shim/gym_minigrid/wrappers.py", "BBAI_ERR_ARG", "BBAI_ERR_STATE", "grid_render_delta", "grid_delta_valid"):
        assert word in text, word


def test_library_exports_the_entries_and_refuses_a_null_handle():
    from babyai_amd import engine
    import __graft_entry__
    __graft_entry__.build()
    import torch  # noqa: F401  (torch's HIP runtime first, as the product loads it)
    lib = engine.bind(ctypes.CDLL(os.path.join(ROOT, "babyai_amd", "libbbai_hip.so")))
    for name in NAMES:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == engine.ABI_GRID_TARGET[name][1]
    assert lib.bbai_set_grid_target(None, None, 8) == -1                          # BBAI_ERR_ARG: null handle
    assert lib.bbai_render_grid_target(None, None) == -1
    assert lib.bbai_step_grid_target(None, None, None, None, None, None, None, 1, None) == -1
    assert lib.bbai_grid_target_invalidate(None) == -1
    assert lib.bbai_grid_target_shadow(None, None, None) == -1
    assert b"null handle" in lib.bbai_last_error()


def test_bind_passes_over_a_library_without_the_entries():
    from babyai_amd import engine

    class Old(object):
        pass
    assert engine.bind(Old()) is not None
    assert engine.BatchedBabyAIEnv._grid_target is False        # a batch has no registered grid target until __init__ finds the entries
