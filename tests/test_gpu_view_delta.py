"""The delta render of the agent's 7x7 view at tile sizes 16 and 32 (k_view_delta, include/bbai.h bbai_set_render_target with the option
"render_target_tile_size"): a whole-batch bbai_render_view into the registered buffer stores only the 64-byte pieces of a frame that show
a cell whose atlas tile changed.  The model is numpy alone: test_view_atlas.view_frames (the frame rule) over the pinned atlases, and the
geometry "byte b of a frame is a colour of pixel b // 3 = (7 ts) y + x, which shows view cell (x // ts) * 7 + y // ts".
  1. chosen dirty cells through the C ABI, the exact footprint: the test overwrites the whole buffer with (the new frame) XOR 0xFF -- which
     differs from the new frame in every byte -- WITHOUT invalidating, so every byte afterwards is either untouched or stored;
  2. live batches against a twin that draws every frame whole (option "render_delta" 0) and against the model, over resets, reseed and
     load_state, at batch sizes that leave a partial last group and less than one group;
  3. what invalidates the shadow, and what does not;
  4. the option's contract, and that tile size 8's delta render neither changed nor takes a 16 target for its own."""
import ctypes

import numpy as np
import pytest

import render_util as ru
from test_view_atlas import load_atlas, view_frames

ROOM = "BabyAI-GoToLocal-v0"
MAZE = "BabyAI-GoTo-v0"
TS = (16, 32)
PIECE = 64
BAND, BAND_BYTE = 256, 0xA5
N1 = 5
_open = []


@pytest.fixture(autouse=True)
def _close_handles():
    yield
    while _open:
        _open.pop().close()


def make_env(gpu, level, n, **kw):
    from babyai_amd.engine import BatchedBabyAIEnv
    e = BatchedBabyAIEnv(level, n, device=gpu, **kw)
    _open.append(e)
    return e


def frame_bytes(ts):
    return 147 * ts * ts


def cell_of_byte(ts):
    p = np.arange(frame_bytes(ts)) // 3
    y, x = p // (7 * ts), p % (7 * ts)
    return (x // ts) * 7 + y // ts


def model_ids(enc, lut):
    """uint8[k, 7, 7, 3] -> uint8[k, 49]: view_frames' rule for the tile of a cell (cell = 7 x + y, the agent's cell (3, 6) has lut row 1)."""
    e = np.asarray(enc).reshape(-1, 49, 3).astype(np.int64)
    key = (e[..., 0] | e[..., 1] << 3 | e[..., 2] << 6) & 255
    row = np.zeros(49, np.int64)
    row[3 * 7 + 6] = 1
    return lut[row[None], key].astype(np.uint8)


def valid(env):
    return env.get_option("render_delta_valid")


def expect_frames(env, ts, what):
    import torch
    torch.cuda.synchronize()
    want = view_frames(env.image.cpu().numpy(), *load_atlas(ts), ts)
    got = env.pixels.cpu().numpy()
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:3].tolist())


# ---- 1. chosen dirty cells, exact footprint -----------------------------------------------------------------------------------------
class Footprint(object):
    """An encoded GoToLocal batch of N1 envs whose handle has the test's own buffer registered as its tile-size-ts target: 256 + N1 F + 256
    bytes, the bands filled with 0xA5, the frames on a 64-byte boundary."""

    def __init__(self, gpu, ts):
        import torch
        self.gpu, self.ts, self.F = gpu, ts, frame_bytes(ts)
        from babyai_amd.engine import BatchedBabyAIEnv
        self.env = env = BatchedBabyAIEnv(ROOM, N1, device=gpu, seeds=1)          # (closed by the module fixture, not per test)
        env._install_atlas("view", ts)
        env.set_option("render_target_tile_size", ts)
        self.raw = torch.full((BAND + N1 * self.F + BAND,), BAND_BYTE, dtype=torch.uint8, device=gpu)
        self.frame = self.raw[BAND:BAND + N1 * self.F]
        assert self.frame.data_ptr() % 64 == 0
        assert env.lib.bbai_set_render_target(env.handle, ctypes.c_void_p(self.frame.data_ptr())) == 0
        assert valid(env) == 0 and env.get_option("render_delta") == 1
        self.tiles, self.lut = load_atlas(ts)
        self.cob = cell_of_byte(ts)

    def render(self, enc):
        import torch
        t = torch.as_tensor(np.ascontiguousarray(enc), device=self.gpu)
        rc = self.env.lib.bbai_render_view(self.env.handle, self.ts, ctypes.c_void_p(t.data_ptr()), N1, None, N1, ctypes.c_void_p(self.frame.data_ptr()),
                                           self.env._stream())
        assert rc == 0, self.env.lib.bbai_last_error()
        torch.cuda.synchronize()
        return self.frame.cpu().numpy()

    def bands_untouched(self):
        return bool(self.raw[:BAND].eq(BAND_BYTE).all()) and bool(self.raw[BAND + N1 * self.F:].eq(BAND_BYTE).all())

    def check(self, enc_a, enc_b, changed):
        """Frame A drawn whole, frame B as a delta render over the poisoned buffer; `changed`: bool[N1, 49], the cells whose tile differs."""
        import torch
        ids_a, ids_b = model_ids(enc_a, self.lut), model_ids(enc_b, self.lut)
        assert np.array_equal(ids_a != ids_b, changed)
        env = self.env
        assert env.lib.bbai_render_invalidate(env.handle) == 0 and valid(env) == 0
        got = self.render(enc_a)
        assert valid(env) == 1
        assert np.array_equal(got, view_frames(enc_a, self.tiles, self.lut, self.ts).reshape(-1))
        assert np.array_equal(env.render_shadow().cpu().numpy(), ids_a)
        new = view_frames(enc_b, self.tiles, self.lut, self.ts).reshape(-1)
        poison = new ^ 0xFF
        self.frame.copy_(torch.as_tensor(poison, device=self.gpu))
        got = self.render(enc_b)
        assert valid(env) == 1
        in_cell = changed[:, self.cob].reshape(-1)                                      # per byte of the buffer: its cell changed
        in_piece = np.repeat(in_cell.reshape(-1, PIECE).any(axis=1), PIECE)            # ... or shares a 64-byte piece with such a byte
        stored = got != poison
        assert np.array_equal(got[in_cell], new[in_cell]), "a byte of a changed cell does not hold the new picture"
        assert not stored[~in_piece].any(), ("stored outside the pieces that touch a changed cell", np.nonzero(stored & ~in_piece)[0][:4].tolist())
        assert np.array_equal(got[stored], new[stored]), "a stored byte that is not the new picture's"
        if not changed.any():
            assert not stored.any()
        assert np.array_equal(env.render_shadow().cpu().numpy(), ids_b)
        assert self.bands_untouched()


@pytest.fixture(scope="module", params=TS)
def footprint(request, gpu):
    f = Footprint(gpu, request.param)
    yield f
    f.env.close()


def cells(*xy):
    return [7 * x + y for x, y in xy]


FOOTPRINT_CASES = {
    "corners": {1: cells((0, 0), (6, 0), (0, 6), (6, 6))},
    "agent_cell": {2: cells((3, 6))},
    "two_side_by_side": {1: cells((2, 3), (3, 3))},
    "two_one_above_the_other": {3: cells((4, 1), (4, 2))},
    "all_cells_of_the_last_env": {N1 - 1: list(range(49))},
    "first_and_last_env": {0: cells((5, 2)), N1 - 1: cells((1, 5))},
    "every_env_something": {0: cells((0, 0)), 1: cells((3, 6), (3, 5)), 2: list(range(0, 49, 5)), 3: cells((6, 6)), 4: cells((0, 3), (6, 3))},
    "nothing": {},
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(FOOTPRINT_CASES))
def test_chosen_dirty_cells_exact_footprint(footprint, case):
    pattern = np.zeros((N1, 49), bool)
    for env, cs in FOOTPRINT_CASES[case].items():
        pattern[env, cs] = True
    enc_a = ru.synthetic_encodings(N1, 100 + len(case))
    enc_b = ru.perturb(enc_a, pattern, seed=7) if pattern.any() else enc_a.copy()
    footprint.check(enc_a, enc_b, pattern)


@pytest.mark.gpu
def test_a_change_that_folds_to_the_same_tile_stores_nothing(footprint):
    """Encoding bytes change, tile ids do not: bit 2 of the state byte leaves the key (o2 << 6 & 255), and two keys of one lut entry."""
    lut = footprint.lut
    enc_a = ru.synthetic_encodings(N1, 55)
    flat_a = enc_a.reshape(N1, 49, 3)
    pair = None
    for ka in range(256):                                # two keys the ordinary cells' table sends to one tile
        same = np.nonzero(lut[0] == lut[0][ka])[0]
        if len(same) > 1:
            pair = (ka, int(same[same != ka][0]))
            break
    assert pair is not None
    unkey = lambda k: (k & 7, (k >> 3) & 7, k >> 6)
    flat_a[2, 10] = unkey(pair[0])
    enc_b = enc_a.copy()
    flat_b = enc_b.reshape(N1, 49, 3)
    flat_b[2, 10] = unkey(pair[1])
    flat_b[0, 0, 2] += 4                                 # (state | 4) << 6 = the same key & 255
    flat_b[N1 - 1, 27, 2] += 4                           # ... in the agent's cell
    flat_b[3, 48, 2] += 8
    assert (enc_a != enc_b).sum() >= 4
    footprint.check(enc_a, enc_b, np.zeros((N1, 49), bool))


# ---- 2. live batches equal the whole-frame render ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("level,ts,n", [(ROOM, 16, 131), (ROOM, 32, 67), (MAZE, 16, 131), (ROOM, 16, 3), (ROOM, 32, 3)])
def test_live_batches_equal_the_whole_frame_render(gpu, level, ts, n):
    import torch
    steps, seed = 80, 500 + ts
    a = make_env(gpu, level, n, seeds=seed, pixel=True, tile_size=ts)
    b = make_env(gpu, level, n, seeds=seed, pixel=True, tile_size=ts)
    assert a.get_option("render_target_tile_size") == ts
    b.set_option("render_delta", 0)
    tiles, lut = load_atlas(ts)

    def same(what):
        torch.cuda.synchronize()
        assert torch.equal(a.image, b.image), what
        assert torch.equal(a.pixels, b.pixels), what
        want = view_frames(a.image.cpu().numpy(), tiles, lut, ts)
        assert np.array_equal(a.pixels.cpu().numpy(), want), what
        assert valid(a) == 1 and valid(b) == 0, what
        assert np.array_equal(a.render_shadow().cpu().numpy(), model_ids(a.image.cpu().numpy(), lut)), what

    a.reset()
    b.reset()
    same("reset")
    rng = np.random.RandomState(n + ts)
    listed = sorted(set([0, n // 2, n - 1]))
    snap = {}
    resets = 0
    for t in range(steps):
        act = torch.as_tensor(rng.randint(0, 7, size=n).astype(np.uint8), device=gpu)
        for e in (a, b):
            e.step(act)
        same(("step", t))
        resets += int(a.done.sum())
        if t == 25:
            for e in (a, b):
                e.reseed(listed, [9000 + i for i in range(len(listed))])
            same("reseed")
        if t == 40:
            snap = {e: e.save_state(listed) for e in (a, b)}
        if t == 60:
            for e in (a, b):
                e.load_state(snap[e], listed)
            same("load_state")
    if level == ROOM and n > 3:
        assert resets > 0                                # episodes ended: whole views changed under the delta render
    assert a.gate_timeouts() == 0


# ---- 3. invalidation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_what_invalidates_the_shadow_and_what_does_not(gpu):
    import torch
    ts, n = 16, 9
    env = make_env(gpu, ROOM, n, seeds=77, pixel=True, tile_size=ts)
    env.reset()
    rng = np.random.RandomState(3)

    def step_and_check(what):
        env.step(torch.as_tensor(rng.randint(0, 7, size=n).astype(np.uint8), device=gpu))
        expect_frames(env, ts, what)
        assert valid(env) == 1, what

    step_and_check("first step")
    flat = env.pixels.view(-1)
    F = frame_bytes(ts)

    # renders elsewhere leave the shadow alone
    env.render_view([0, 1])
    env.render_view([2], tile_size=32)
    env.render_view(tile_size=8)                         # (installs the tile-size-8 atlas: bbai_set_atlas is not this target's atlas)
    env.render_encoding(env.image[:2].contiguous(), tile_size=32)
    env.render_encoding(out=torch.empty((n, 7 * ts, 7 * ts, 3), dtype=torch.uint8, device=gpu))
    assert valid(env) == 1
    step_and_check("after renders elsewhere")

    # listed ids into a slice of the registered buffer
    env.render_view(ids=[0, 1], out=env.pixels[2:4])
    assert valid(env) == 0
    step_and_check("render_view(ids) into a slice")
    # a partial count into its start
    env.render_encoding(env.image[:4].contiguous(), out=env.pixels[:4])
    assert valid(env) == 0
    step_and_check("a partial count")
    # another tile size into an overlapping buffer: 32 over the start, 8 behind the first n * 9408 bytes
    env.render_encoding(env.image[:2].contiguous(), out=flat[:2 * frame_bytes(32)].view(2, 224, 224, 3), tile_size=32)
    assert valid(env) == 0
    step_and_check("tile size 32 into the buffer")
    off = n * ru.PIX_BYTES
    assert off % 16 == 0 and off + n * ru.PIX_BYTES <= n * F
    env.render_encoding(out=flat[off:off + n * ru.PIX_BYTES].view(n, 56, 56, 3), tile_size=8)
    assert valid(env) == 0
    step_and_check("tile size 8 into the buffer, past n * 9408 bytes")
    env.render_invalidate()
    assert valid(env) == 0
    step_and_check("bbai_render_invalidate")
    env._atlases.discard(("view", ts))
    env._install_atlas("view", ts)
    assert valid(env) == 0
    step_and_check("the view atlas installed again")
    env.set_option("render_delta", 0)
    assert valid(env) == 0
    env.step(torch.as_tensor(rng.randint(0, 7, size=n).astype(np.uint8), device=gpu))
    expect_frames(env, ts, "render_delta 0")
    assert valid(env) == 0
    env.set_option("render_delta", 1)
    assert valid(env) == 0
    step_and_check("render_delta back at 1")
    env.pixels.fill_(7)
    env.render_invalidate()
    assert valid(env) == 0
    step_and_check("the caller's own write + bbai_render_invalidate")
    step_and_check("one more")


# ---- 4. the option's contract ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_option_contract(gpu):
    from babyai_amd.engine import EngineError
    env = make_env(gpu, ROOM, 4, seeds=1)
    assert env.get_option("render_target_tile_size") == 8
    for v in (16, 32, 8):
        env.set_option("render_target_tile_size", v)
        assert env.get_option("render_target_tile_size") == v
    for v in (12, 0, -1, 64):
        with pytest.raises(EngineError):
            env.set_option("render_target_tile_size", v)
        assert env.get_option("render_target_tile_size") == 8


@pytest.mark.gpu
def test_tile_size_8_takes_the_delta_path_it_took(gpu):
    import torch
    n = 130
    env = make_env(gpu, ROOM, n, seeds=40, pixel=True)
    assert env.get_option("render_target_tile_size") == 8
    env.reset()
    rng = np.random.RandomState(8)
    for t in range(21):
        torch.cuda.synchronize()
        ids = ru.tile_ids(env.image.cpu().numpy())
        assert valid(env) == 1
        assert np.array_equal(env.pixels.cpu().numpy(), ru.frames(ids)), t
        assert np.array_equal(env.render_shadow().cpu().numpy(), ids), t
        env.step(torch.as_tensor(rng.randint(0, 7, size=n).astype(np.uint8), device=gpu))


@pytest.mark.gpu
def test_the_tile_size_8_planner_leaves_a_16_target_alone(gpu):
    import torch
    n, ts = 16, 16
    env = make_env(gpu, ROOM, n, seeds=3)
    env.reset()
    env._install_atlas("view", 8)
    env._install_atlas("view", ts)
    env.set_option("render_target_tile_size", ts)
    target = torch.zeros((n, 7 * ts, 7 * ts, 3), dtype=torch.uint8, device=gpu)
    lib, h = env.lib, env.handle
    assert lib.bbai_set_render_target(h, ctypes.c_void_p(target.data_ptr())) == 0
    env.render_encoding(out=target, tile_size=ts)
    assert valid(env) == 1
    want16 = view_frames(env.image.cpu().numpy(), *load_atlas(ts), ts)
    assert np.array_equal(target.cpu().numpy(), want16)
    env.step(torch.as_tensor(np.random.RandomState(1).randint(0, 7, size=n).astype(np.uint8), device=gpu))
    want8 = ru.frames(ru.tile_ids(env.image.cpu().numpy()))
    # bbai_render into a buffer of its own: a plain full render, and the 16 target's shadow stays valid
    out8 = torch.full((n, 56, 56, 3), 0x5A, dtype=torch.uint8, device=gpu)
    assert lib.bbai_render(h, ctypes.c_void_p(env.image.data_ptr()), ctypes.c_void_p(out8.data_ptr()), env._stream()) == 0
    assert np.array_equal(out8.cpu().numpy(), want8)
    assert valid(env) == 1
    # ... and into the registered buffer's first n * 9408 bytes: still every byte (the shadow holds ids of another frame size), shadow dropped
    head = target.view(-1)[:n * ru.PIX_BYTES]
    head.fill_(0x5A)
    assert lib.bbai_render(h, ctypes.c_void_p(env.image.data_ptr()), ctypes.c_void_p(head.data_ptr()), env._stream()) == 0
    assert np.array_equal(head.cpu().numpy().reshape(n, 56, 56, 3), want8)
    assert valid(env) == 0
    # bbai_step_render with that pointer: as if no target were registered
    act = torch.as_tensor(np.random.RandomState(2).randint(0, 7, size=n).astype(np.uint8), device=gpu)
    env.set_option("render_delta_from_step", 1)
    head.fill_(0x5A)
    assert lib.bbai_step_render(h, ctypes.c_void_p(act.data_ptr()), *[ctypes.c_void_p(p) for p in env._out_ptrs], 1, ctypes.c_void_p(head.data_ptr()), env._stream()) == 0
    assert np.array_equal(head.cpu().numpy().reshape(n, 56, 56, 3), ru.frames(ru.tile_ids(env.image.cpu().numpy())))
    env.render_encoding(out=target, tile_size=ts)
    assert valid(env) == 1
    assert np.array_equal(target.cpu().numpy(), view_frames(env.image.cpu().numpy(), *load_atlas(ts), ts))


@pytest.mark.gpu
def test_a_tile_size_16_render_into_an_8_target_drops_its_shadow(gpu):
    """The mirror: a frame at 16 written into the head of the buffer registered at 8 (16 x 9408 B: room for four such frames)."""
    import torch
    n = 16
    env = make_env(gpu, ROOM, n, seeds=5, pixel=True)
    env.reset()
    rng = np.random.RandomState(4)
    env.step(torch.as_tensor(rng.randint(0, 7, size=n).astype(np.uint8), device=gpu))
    assert valid(env) == 1
    F = frame_bytes(16)
    assert F == 37632 and F <= n * ru.PIX_BYTES
    head = env.pixels.view(-1)[:F].view(1, 112, 112, 3)
    enc = env.image[:1].contiguous()
    env.render_encoding(enc, out=head, tile_size=16)
    torch.cuda.synchronize()
    assert np.array_equal(head.cpu().numpy(), view_frames(enc.cpu().numpy(), *load_atlas(16), 16))
    assert valid(env) == 0
    env.step(torch.as_tensor(rng.randint(0, 7, size=n).astype(np.uint8), device=gpu))
    torch.cuda.synchronize()
    assert np.array_equal(env.pixels.cpu().numpy(), ru.frames(ru.tile_ids(env.image.cpu().numpy())))
    assert valid(env) == 1
