"""The registered full-grid target on the device (include/bbai_grid_target.h; k_grid_delta<TS>, k_grid_ids): a full_obs pixel batch keeps
`full` current by storing only the 64-byte pieces that hold a changed cell.

1. Twin batches -- the same seeds and actions with the delta render on and off ("grid_render_delta") -- hold byte-equal frames after
   reset() and every step, through step(), rollout(), load_state() and reseed(), and the shadow is the tile ids of the twin's frames.
2. The exact store footprint, by the method of tests/test_gpu_render_delta_footprint.py: the test owns the registered buffer (256-byte
   bands of 0xA5 on both sides) and before every delta render overwrites the frames with Q = 255 - (the new frame), which differs from
   it in every byte; afterwards every piece of grid_delta_util.stored_mask holds the new frame, every other byte Q, the bands are
   untouched.  The dirty cells come from chosen actions on real states, and the cases the test exists for are asserted to occur.
   (Two cases cannot occur and are asserted in the form that can: no piece spans two TILE rows -- a tile row is 3 W ts^2 bytes, a whole
   number of pieces; the host test proves it -- so it is dirty pieces spanning two PIXEL rows on the 4 x 4 and 22 x 22 grids; and walls
   never change, so no real transition dirties half of an env's cells: it is three or more changed cells in several tile rows.)
3. What drops the history, and what does not.
4. The refusals.
The reference side (grid_delta_util) is pinned without a GPU in tests/test_grid_delta_host.py."""
import ctypes

import numpy as np
import pytest

import grid_delta_util as gdu

LEVELS = {"BabyAI-GoToObjS4-v0": (4, 4), "BabyAI-KeyCorridorS3R1-v0": (7, 3), "BabyAI-GoToLocal-v0": (8, 8), "BabyAI-BossLevel-v0": (22, 22)}
BOSS, ROOM, SMALL = "BabyAI-BossLevel-v0", "BabyAI-GoToLocal-v0", "BabyAI-GoToObjS4-v0"
TWINS = [(level, ts, n) for level in LEVELS for ts in gdu.TILE_SIZES for n in (1, 3)] + [(BOSS, 32, 130)]
BAND, BAND_BYTE = 256, 0xA5
# envs per group of k_grid_delta (option "grid_delta_group"; 0 = by batch size: ONE below 1 024 envs on 256 CUs).  The cases at n = 130 run
# at 8 and 32 as well (32 is clamped to 8 on BossLevel): two and a quarter / sixteen and a quarter groups, the last one partial; the large
# batches below reach the same shapes through the default.
GROUPS = (0, 8, 32)
# (level, tile size, n): default group size -- n / blocks envs -- 32 with a partial last group, 8 likewise, and 4 (between 1 and the cap)
LARGE = [(ROOM, 8, 512 * 32 + 13), (BOSS, 8, 4096 + 5), (ROOM, 8, 2048 + 3)]
# after env i has loaded env i + 1's state: two independent layouts of D objects and the agent differ in up to 2 (D + 1) cells; some env of the
# batch must show at least half of that (GoToLocal D = 8, BossLevel D = 18 before its doors; the two small levels: agent and one object)
ROTATED_CELLS = {SMALL: 3, "BabyAI-KeyCorridorS3R1-v0": 3, ROOM: 9, BOSS: 19}
ERR_ARG, ERR_STATE = -1, -3
LEFT, FORWARD = 0, 2
_open = []


@pytest.fixture(autouse=True)
def _close_handles():
    yield
    while _open:
        _open.pop().close()
    import gc
    gc.collect()
    try:
        import torch
        torch.cuda.empty_cache()
    except Exception:
        pass


def make_env(gpu, level, n, ts, seed=77, **kw):
    from babyai_amd.engine import BatchedBabyAIEnv
    kw.setdefault("full_obs", True)
    e = BatchedBabyAIEnv(level, n, device=gpu, seeds=seed, pixel=True, tile_size=ts, **kw)
    _open.append(e)
    return e


def whole(env, ts):
    """The frames of the current state drawn whole into a buffer of their own: render('rgb_array', highlight=False)."""
    return env.render_grid(None, tile_size=ts, highlight=False)


def poisoned(env, ts):
    """env.full overwritten with Q = 255 - (the frames of the current state); returns those frames."""
    want = whole(env, ts)
    env.full.copy_(255 - want)
    return want


# ---- 1. twin batches ----------------------------------------------------------------------------------------------------------------
def group_cap(env):
    """What griddelta_group gives for the env's grid (tests/test_grid_delta_host.py pins the header's to this arithmetic)."""
    c = env.cfg
    return max(1, min(32, 4096 // (c.W * c.H), 2048 // (c.H * c.ES // 4)))


def default_group(env, gpu):
    import torch
    blocks = 2 * torch.cuda.get_device_properties(gpu).multi_processor_count
    return max(1, min(group_cap(env), env.num_envs // blocks))


def twins(gpu, level, n, ts, group=0, **kw):
    a, b = make_env(gpu, level, n, ts, **kw), make_env(gpu, level, n, ts, **kw)
    assert a._grid_target and b._grid_target
    assert a.get_option("grid_render_delta") == 1 and a.get_option("grid_delta_valid") == 0 and a.get_option("grid_delta_group") == 0
    a.set_option("grid_delta_group", group)
    assert a.get_option("grid_delta_group") == group
    b.set_option("grid_render_delta", 0)
    assert b.get_option("grid_render_delta") == 0
    return a, b


def same(a, b, ts, where):
    import torch
    assert a.get_option("grid_delta_valid") == 1 and b.get_option("grid_delta_valid") == 1, where
    assert torch.equal(a.full, b.full), where
    want = gdu.frame_ids_device(b.full, ts)
    assert torch.equal(a.grid_shadow(), want) and torch.equal(b.grid_shadow(), want), where


@pytest.mark.gpu
@pytest.mark.parametrize("level,ts,n", TWINS)
def test_twin_batches_hold_the_same_frames(gpu, level, ts, n):
    import torch
    a, b = twins(gpu, level, n, ts)
    W, H = LEVELS[level]
    assert tuple(a.full.shape) == (n, H * ts, W * ts, 3)
    acts = torch.as_tensor(np.random.RandomState(n + ts).randint(0, 7, size=(40, n)).astype(np.uint8), device=gpu)
    oa, ob = a.reset(), b.reset()
    assert oa["image"].data_ptr() == a.full.data_ptr()
    same(a, b, ts, "reset")
    for t in range(40):
        oa = a.step(acts[t])[0]
        b.step(acts[t])
        assert oa["image"].data_ptr() == a.full.data_ptr()
        same(a, b, ts, t)
    assert torch.equal(a.full, whole(a, ts))             # ... which are the frames of the state


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS[1:] + (5,))
@pytest.mark.parametrize("level,ts", [(SMALL, 8), ("BabyAI-KeyCorridorS3R1-v0", 16), (ROOM, 8), (BOSS, 8), (BOSS, 32)])
def test_twin_batches_with_several_envs_per_group(gpu, level, ts, group):
    """n = 130 with 8, 32 and 5 envs per group: whole groups and a partial last one (130 = 16 x 8 + 2 = 4 x 32 + 2 = 26 x 5)."""
    import torch
    n = 130
    a, b = twins(gpu, level, n, ts, group=group)
    g = min(group, group_cap(a))
    assert g > 1 and (n % g != 0 or group == 5)
    acts = torch.as_tensor(np.random.RandomState(group + ts).randint(0, 7, size=(24, n)).astype(np.uint8), device=gpu)
    a.reset(), b.reset()
    same(a, b, ts, "reset")
    for t in range(24):
        a.step(acts[t]), b.step(acts[t])
        same(a, b, ts, t)
    assert torch.equal(a.full, whole(a, ts))


@pytest.mark.gpu
@pytest.mark.parametrize("level,ts,n", LARGE)
def test_twin_batches_at_the_default_group_size(gpu, level, ts, n):
    """Batches large enough that the default launch takes several envs per group -- the cap with a partial last group, and a size between 1
    and the cap -- which is the shape of every measured workload."""
    import torch
    a, b = twins(gpu, level, n, ts)
    G, cap = default_group(a, gpu), group_cap(a)
    assert G > 1 and n % G != 0 and (G == cap or n < 4096), (G, cap)
    acts = torch.as_tensor(np.random.RandomState(n % 1000).randint(0, 7, size=(10, n)).astype(np.uint8), device=gpu)
    a.reset(), b.reset()
    same(a, b, ts, "reset")
    for t in range(10):
        a.step(acts[t]), b.step(acts[t])
        same(a, b, ts, t)
    assert torch.equal(a.full, whole(a, ts))


@pytest.mark.gpu
def test_twin_batches_with_frozen_envs(gpu):
    import torch
    a, b = twins(gpu, ROOM, 130, 8, group=8, auto_reset=False)
    acts = torch.as_tensor(np.random.RandomState(5).choice([0, 1, 2, 2, 2, 3, 5], size=(40, 130)).astype(np.uint8), device=gpu)
    a.reset(), b.reset()
    same(a, b, 8, "reset")
    frozen = 0
    for t in range(40):
        _, _, done, _ = a.step(acts[t])
        b.step(acts[t])
        frozen += int(done.sum())
        same(a, b, 8, t)
    assert frozen > 0
    a.reset(), b.reset()
    same(a, b, 8, "second reset")


@pytest.mark.gpu
def test_twin_batches_through_rollout_load_state_and_reseed(gpu):
    import torch
    n, ts = 130, 16
    a, b = twins(gpu, ROOM, n, ts, group=32)
    rng = np.random.RandomState(9)
    acts = torch.as_tensor(rng.randint(0, 7, size=(24, n)).astype(np.uint8), device=gpu)
    a.reset(), b.reset()
    oa = a.rollout(acts[:12])
    b.rollout(acts[:12])
    assert oa["image"].data_ptr() == a.full.data_ptr()
    same(a, b, ts, "rollout")
    snaps = a.save_state(), b.save_state()
    a.rollout(acts[12:]), b.rollout(acts[12:])
    same(a, b, ts, "second rollout")
    ids = [3, 64, 65, 129, 7]
    rows = [4, 0, 129, 64, 7]
    for env, snap in zip((a, b), snaps):
        env.load_state(snap, ids, rows)
    same(a, b, ts, "load_state")
    assert torch.equal(a.full, whole(a, ts))
    for env in (a, b):
        env.reseed([0, 63, 64, 128], [1001, 1002, 1003, 1004])
    same(a, b, ts, "reseed")
    assert torch.equal(a.full, whole(a, ts))
    for t in range(4):
        a.step(acts[t]), b.step(acts[t])
        same(a, b, ts, "step %d behind reseed" % t)


# ---- 2. the exact store footprint ---------------------------------------------------------------------------------------------------
class Target(object):
    """The test's own grid target: one allocation of 256 + n * F + 256 bytes, the frames on a 64-byte boundary and registered with the
    handle, both bands filled with 0xA5."""

    def __init__(self, env, gpu, ts):
        import torch
        self.n, self.F = env.num_envs, gdu.frame_bytes(env.cfg.W, env.cfg.H, ts)
        self.raw = torch.full((BAND + self.n * self.F + BAND,), BAND_BYTE, dtype=torch.uint8, device=gpu)
        self.frame = self.raw[BAND:BAND + self.n * self.F]
        assert self.frame.data_ptr() % 64 == 0
        assert env.lib.bbai_set_grid_target(env.handle, ctypes.c_void_p(self.frame.data_ptr()), ts) == 0
        assert env.get_option("grid_render_delta") == 1 and env.get_option("grid_delta_valid") == 0

    def bands_untouched(self):
        return bool(self.raw[:BAND].eq(BAND_BYTE).all()) and bool(self.raw[BAND + self.n * self.F:].eq(BAND_BYTE).all())


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("ts", gdu.TILE_SIZES)
@pytest.mark.parametrize("level", list(LEVELS))
def test_exact_store_footprint(gpu, level, ts, group):
    footprint(gpu, level, ts, 130, group)


@pytest.mark.gpu
@pytest.mark.parametrize("level,ts,n", LARGE)
def test_exact_store_footprint_at_the_default_group_size(gpu, level, ts, n):
    footprint(gpu, level, ts, n, 0)


def footprint(gpu, level, ts, n, group):
    import torch
    W, H = LEVELS[level]
    env = make_env(gpu, level, n, ts)
    env.set_option("grid_delta_group", group)
    G = min(group, group_cap(env)) if group else default_group(env, gpu)
    assert n % G != 0 or G == 1                       # (several envs per group: the last group is partial)
    assert (n > 130) == (G > 1 and group == 0)
    target = Target(env, gpu, ts)
    env._grid_target = False          # from here on the batch's own calls draw `full` whole (bbai_render_grid): the new frame of every transition
    env.set_option("step_hold", 1)
    inc = torch.as_tensor(gdu.piece_cells(W, H, ts).T.astype(np.float32), device=gpu)            # [H W, NP]
    rb = 3 * W * ts
    two_rows = torch.as_tensor((np.arange(inc.shape[1]) * 64) // rb != (np.arange(inc.shape[1]) * 64 + 63) // rb, device=gpu)

    def render():
        assert env.lib.bbai_render_grid_target(env.handle, env._stream()) == 0
        assert env.get_option("grid_delta_valid") == 1

    env.reset()
    render()                                              # no history: whole frames, the shadow behind them
    assert torch.equal(target.frame, env.full.view(-1)) and target.bands_untouched()
    ids = gdu.frame_ids_device(env.full, ts)
    assert torch.equal(env.grid_shadow(), ids)
    seen = dict(none=0, one=0, hor=0, ver=0, two_rows=0, many=0, clean_block=0, max_share=0.0, max_cells=0)

    def transition(change, what):
        """`change` moves the state (and draws the new frames whole into env.full); then one delta render into the Q-poisoned target."""
        nonlocal ids
        before = ids
        change()
        new = env.full
        after = gdu.frame_ids_device(new, ts)
        q = (255 - new).view(-1)
        target.frame.copy_(q)
        render()
        changed = (before != after)
        mask = (changed.float() @ inc) > 0                                             # [n, NP]: grid_delta_util.stored_mask, on the device
        if n * inc.shape[1] <= 1 << 16:
            assert np.array_equal(mask.cpu().numpy(), gdu.stored_mask(before.cpu().numpy(), after.cpu().numpy(), W, H, ts))
        want = torch.where(mask.repeat_interleave(64, dim=1).view(-1), new.view(-1), q)
        if not torch.equal(target.frame, want):
            got = target.frame
            extra = ((got != q) & ~mask.repeat_interleave(64, dim=1).view(-1)).nonzero().view(-1)
            missing = ((got != new.view(-1)) & mask.repeat_interleave(64, dim=1).view(-1)).nonzero().view(-1)
            raise AssertionError((level, ts, what, "bytes stored outside the mask", int(extra.numel()), extra[:4].tolist(),
                                  "bytes of the mask not stored or wrong", int(missing.numel()), missing[:4].tolist()))
        assert target.bands_untouched(), (level, ts, what)
        assert torch.equal(env.grid_shadow(), after), (level, ts, what)
        ids = after
        # what this transition showed
        cnt = changed.sum(dim=1)
        ch = changed.view(n, H, W)
        seen["none"] += int((cnt == 0).sum())
        seen["one"] += int((cnt == 1).sum())
        hor = (cnt == 2) & (ch[:, :, :-1] & ch[:, :, 1:]).any(dim=2).any(dim=1)
        ver = (cnt == 2) & (ch[:, :-1, :] & ch[:, 1:, :]).any(dim=2).any(dim=1)
        # two horizontal neighbours share a piece: some piece holds bytes of both, i.e. fewer dirty pieces than the two cells' own counts
        per_cell = (inc > 0).sum(dim=1).float()                                       # pieces per cell
        shared = mask.sum(dim=1).float() < (changed.float() @ per_cell)
        seen["hor"] += int((hor & shared).sum())
        seen["ver"] += int(ver.sum())
        seen["two_rows"] += int((mask & two_rows[None, :]).sum())
        rows_hit = ch.any(dim=2).sum(dim=1)
        seen["many"] += int(((cnt >= 3) & ((rows_hit >= 2) | (H == 3))).sum())
        seen["clean_block"] += int((cnt[:64] == 0).all() and (cnt[64:] > 0).any())
        seen["max_share"] = max(seen["max_share"], float(mask.float().mean(dim=1).max()))
        seen["max_cells"] = max(seen["max_cells"], int(cnt.max()))
        return cnt

    def act(a, first=0):
        acts = torch.full((n,), env.HOLD, dtype=torch.uint8, device=gpu)
        acts[first:] = a
        return lambda: env.step(acts)

    snap = env.save_state()
    cnt = transition(act(env.HOLD), "everybody holds")
    assert int(cnt.sum()) == 0
    # (a turn changes the agent's cell, a move two neighbouring cells or none -- but for the envs whose mission that very action completes:
    # they start a new level)
    cnt = transition(act(LEFT), "everybody turns left")
    assert int((cnt == 1).sum()) >= n // 2
    for k in range(3):
        cnt = transition(act(FORWARD), "everybody moves forward (%d)" % k)
        assert int(((cnt == 0) | (cnt == 2)).sum()) >= n // 2
        cnt = transition(act(LEFT), "everybody turns left (%d)" % k)
        assert int((cnt == 1).sum()) >= n // 2
    cnt = transition(lambda: env.load_state(snap, list(range(n)), [(i + 1) % n for i in range(n)]), "env i loads the state of env i + 1")
    assert int(cnt.max()) >= ROTATED_CELLS[level], (level, int(cnt.max()))       # the env with the most dirty cells: its rows shared by all waves
    transition(act(LEFT, 64), "the first 64 envs hold, the rest turn")
    transition(act(FORWARD, 64), "the first 64 envs hold, the rest move")
    print(level, ts, n, "G =", G, seen)
    # the cases this test exists for (a failed precondition is an error of the test, not a skip)
    assert seen["none"] > 0 and seen["one"] > 0 and seen["clean_block"] >= 1, seen
    if H > 3:
        assert seen["ver"] > 0, seen                     # (7 x 3: one row of floor, nothing moves vertically)
    if ts == 8:
        assert seen["hor"] > 0, seen
    if ts == 8 and level in (SMALL, BOSS):
        assert seen["two_rows"] > 0, seen                # dirty pieces that span two PIXEL rows (no piece spans two tile rows: the host test)
    assert seen["many"] > 0, seen                        # the loaded states: an env with three or more changed cells, in several tile rows where the grid has them


# ---- 3. invalidation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_what_drops_the_history(gpu):
    import torch
    n, ts = 5, 8
    env = make_env(gpu, ROOM, n, ts)
    env.reset()
    acts = torch.zeros((n,), dtype=torch.uint8, device=gpu)

    def restored(what):
        assert env.get_option("grid_delta_valid") == 0, what
        want = poisoned(env, ts)
        env.observe_full()
        assert torch.equal(env.full, want), what         # every byte rewritten: the frames were drawn whole
        assert env.get_option("grid_delta_valid") == 1, what
        env.step(acts)
        assert env.get_option("grid_delta_valid") == 1 and torch.equal(env.full, whole(env, ts)), what

    def kept(what):
        assert env.get_option("grid_delta_valid") == 1, what
        want = poisoned(env, ts)
        env.observe_full()                               # a delta render of an unchanged state: stores nothing
        assert torch.equal(env.full, 255 - want), what
        env.full.copy_(want)

    assert env.get_option("grid_delta_valid") == 1
    kept("nothing happened")
    env.render_invalidate()
    restored("render_invalidate")
    env._atlases.discard(("grid", ts))
    env._install_atlas("grid", ts)
    restored("the atlas of the registered tile size installed again")
    env.render_grid([0], tile_size=ts, highlight=False, out=env.full[1:2])
    restored("render_grid into the registered buffer")
    env.render_grid([0], tile_size=ts, highlight=True, out=env.full[n - 1:])
    restored("render_grid into the registered buffer's last frame")
    env.observe_view([0, 1], view_size=5, out=env.full.view(-1)[64:64 + 2 * 75].view(2, 5, 5, 3))
    restored("observe_view into the registered buffer")
    env.observe_full([2], out=env.full[2:3])             # (listed envs: bbai_render_grid into the registered buffer)
    restored("observe_full of listed envs into the registered buffer")
    assert env.lib.bbai_set_grid_target(env.handle, ctypes.c_void_p(env.full.data_ptr()), ts) == 0
    restored("registered again")
    # ... and what does not
    env.render_grid([0, 1], tile_size=ts, highlight=True)
    kept("render_grid into a buffer of its own")
    env.render_grid([0], tile_size=16, highlight=False)              # installs the atlas of another tile size
    env._atlases.discard(("grid", 16))
    env._install_atlas("grid", 16)
    kept("the atlas of another tile size installed")
    env.observe_view([0, 1], view_size=5)
    kept("observe_view into a buffer of its own")
    snap = env.save_state()
    env.load_state(snap)
    assert env.get_option("grid_delta_valid") == 1


@pytest.mark.gpu
def test_grid_target_and_view_target_side_by_side(gpu):
    """A pixel=True 7x7 batch registers `pixels` as the 7x7 target; the caller registers a grid target next to it.  Each keeps its history
    through the other's renders, and a render of either into the other's buffer drops exactly the other's."""
    import torch
    n, ts = 6, 8
    env = make_env(gpu, SMALL, n, ts, full_obs=False)
    assert not env._grid_target and env.pixels is not None
    env._install_atlas("grid", ts)
    F = gdu.frame_bytes(4, 4, ts)
    buf = torch.zeros((n * 9408,), dtype=torch.uint8, device=gpu)          # the grid frames in front, room for n 7x7 frames
    lib, h = env.lib, env.handle
    assert lib.bbai_set_grid_target(h, ctypes.c_void_p(buf.data_ptr()), ts) == 0
    acts = torch.full((n,), LEFT, dtype=torch.uint8, device=gpu)
    env.reset()
    env.step(acts)
    assert lib.bbai_render_grid_target(h, env._stream()) == 0
    assert env.get_option("render_delta_valid") == 1 and env.get_option("grid_delta_valid") == 1
    for _ in range(2):
        env.step(acts)
        assert lib.bbai_render_grid_target(h, env._stream()) == 0
        assert env.get_option("render_delta_valid") == 1 and env.get_option("grid_delta_valid") == 1
    assert torch.equal(buf[:n * F].view(n, 4 * ts, 4 * ts, 3), whole(env, ts))
    # the 7x7 frames into the grid target's buffer: its history goes, the 7x7 target's stays
    assert lib.bbai_render(h, ctypes.c_void_p(env.image.data_ptr()), ctypes.c_void_p(buf.data_ptr()), env._stream()) == 0
    assert env.get_option("grid_delta_valid") == 0 and env.get_option("render_delta_valid") == 1
    assert lib.bbai_render_grid_target(h, env._stream()) == 0
    assert env.get_option("grid_delta_valid") == 1 and torch.equal(buf[:n * F].view(n, 4 * ts, 4 * ts, 3), whole(env, ts))
    # the grid target laid over the 7x7 target's buffer: a render into it drops the 7x7 history, and keeps its own
    assert env.pixels.data_ptr() % 64 == 0
    assert lib.bbai_set_grid_target(h, ctypes.c_void_p(env.pixels.data_ptr()), ts) == 0
    assert env.get_option("render_delta_valid") == 1 and env.get_option("grid_delta_valid") == 0
    assert lib.bbai_render_grid_target(h, env._stream()) == 0
    assert env.get_option("render_delta_valid") == 0 and env.get_option("grid_delta_valid") == 1
    assert torch.equal(env.pixels.view(-1)[:n * F].view(n, 4 * ts, 4 * ts, 3), whole(env, ts))
    assert lib.bbai_set_grid_target(h, None, ts) == 0
    env.step(acts)                                        # the 7x7 render draws its frames whole again
    assert env.get_option("render_delta_valid") == 1


POISON = 0x5A


def view_restored(env, acts, what):
    """The 7x7 target's history is gone: the next step() draws every frame whole (every byte of poisoned `pixels` rewritten) and restores it."""
    import torch
    assert env.get_option("render_delta_valid") == 0, what
    env.pixels.fill_(POISON)
    env.step(acts)
    assert torch.equal(env.pixels, env.render_encoding(out=torch.empty_like(env.pixels))), what
    assert env.get_option("render_delta_valid") == 1, what


@pytest.mark.gpu
def test_listed_frames_into_the_view_target_drop_its_history(gpu):
    """bbai_render_grid, bbai_observe_view and bbai_observe_full write listed envs' frames wherever the caller says: into the bytes of the
    registered 7x7 target they drop its history, as into the grid target's (test_what_drops_the_history); elsewhere they leave it."""
    import torch
    n, ts = 6, 8
    env = make_env(gpu, SMALL, n, ts, full_obs=False)
    env._install_atlas("grid", ts)
    acts = torch.full((n,), LEFT, dtype=torch.uint8, device=gpu)
    env.reset()
    env.step(acts)
    assert env.get_option("render_delta_valid") == 1
    flat = env.pixels.view(-1)
    assert flat.data_ptr() % 16 == 0 and flat.numel() == n * 9408

    def kept(what):
        assert env.get_option("render_delta_valid") == 1, what
        env.step(acts)                                    # a delta render
        assert env.get_option("render_delta_valid") == 1 and torch.equal(env.pixels, env.render_encoding(out=torch.empty_like(env.pixels))), what

    env.render_grid([0], tile_size=ts, out=flat[9408:9408 + 3072].view(1, 32, 32, 3))             # the second frame's first bytes
    view_restored(env, acts, "render_grid into the registered buffer")
    env.observe_view([0, 1], view_size=5, out=flat[64:64 + 2 * 75].view(2, 5, 5, 3))
    view_restored(env, acts, "observe_view into the registered buffer")
    env.observe_full([2], out=flat[n * 9408 - 48:].view(1, 4, 4, 3))                             # the buffer's last 48 bytes
    view_restored(env, acts, "observe_full into the registered buffer")
    env.render_grid([0], tile_size=ts)
    kept("render_grid into a buffer of its own")
    env.observe_view([0, 1], view_size=5)
    kept("observe_view into a buffer of its own")
    env.observe_full([2])
    kept("observe_full into a buffer of its own")


@pytest.mark.gpu
def test_step_full_and_step_view_tell_both_targets(gpu):
    """bbai_step_view / bbai_step_full write n frames to a buffer the caller names: inside a registered buffer they drop that target's
    history and leave the other's, and the next render of the dropped one rewrites every byte."""
    import torch
    n, ts = 6, 8
    env = make_env(gpu, SMALL, n, ts, full_obs=False)
    env._install_atlas("grid", ts)
    F = gdu.frame_bytes(4, 4, ts)
    buf = torch.zeros((n * F,), dtype=torch.uint8, device=gpu)
    lib, h = env.lib, env.handle
    assert lib.bbai_set_grid_target(h, ctypes.c_void_p(buf.data_ptr()), ts) == 0
    acts = torch.full((n,), LEFT, dtype=torch.uint8, device=gpu)
    valid = lambda: (env.get_option("render_delta_valid"), env.get_option("grid_delta_valid"))
    grid_frames = lambda: buf.view(n, 4 * ts, 4 * ts, 3)
    env.reset()
    env.step(acts)
    assert lib.bbai_render_grid_target(h, env._stream()) == 0
    assert valid() == (1, 1)
    # the 5x5 views of a step into the grid target's buffer
    view = buf[64:64 + n * 75]
    assert view.data_ptr() % 16 == 0
    assert lib.bbai_step_view(h, acts.data_ptr(), *env._step_out(), 5, view.data_ptr(), env._stream()) == 0
    assert valid() == (1, 0)
    buf.fill_(POISON)
    assert lib.bbai_render_grid_target(h, env._stream()) == 0
    assert valid() == (1, 1) and torch.equal(grid_frames(), whole(env, ts))
    env.step(acts)                                        # the untouched 7x7 target: a delta render, of two steps' changes
    assert valid() == (1, 1) and torch.equal(env.pixels, env.render_encoding(out=torch.empty_like(env.pixels)))
    # a step's full observations into the 7x7 target's buffer
    full = env.pixels.view(-1)[128:128 + n * 48]
    assert full.data_ptr() % 16 == 0
    assert lib.bbai_step_full(h, acts.data_ptr(), *env._step_out(), full.data_ptr(), env._stream()) == 0
    assert valid() == (0, 1)
    view_restored(env, acts, "bbai_step_full into the registered buffer")
    assert lib.bbai_render_grid_target(h, env._stream()) == 0                # the untouched grid target: a delta render
    assert valid() == (1, 1) and torch.equal(grid_frames(), whole(env, ts))
    # buffers of their own: both histories stay
    own = torch.empty((n * 75,), dtype=torch.uint8, device=gpu)
    assert lib.bbai_step_view(h, acts.data_ptr(), *env._step_out(), 5, own.data_ptr(), env._stream()) == 0
    assert lib.bbai_step_full(h, acts.data_ptr(), *env._step_out(), own.data_ptr(), env._stream()) == 0
    assert valid() == (1, 1)


# ---- 4. errors ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(gpu):
    import torch
    n, ts = 4, 8
    env = make_env(gpu, ROOM, n, ts)
    lib, h = env.lib, env.handle
    valid = lambda: env.get_option("grid_delta_valid")
    # before reset
    assert lib.bbai_render_grid_target(h, env._stream()) == ERR_STATE and b"before reset" in lib.bbai_last_error() and valid() == 0
    acts = torch.zeros((n,), dtype=torch.uint8, device=gpu)
    assert lib.bbai_step_grid_target(h, ctypes.c_void_p(acts.data_ptr()), *env._step_out(), env._stream()) == ERR_STATE and valid() == 0
    env.reset()
    assert valid() == 1
    # a refused registration registers nothing
    assert lib.bbai_set_grid_target(h, ctypes.c_void_p(env.full.data_ptr() + 16), ts) == ERR_ARG and b"aligned" in lib.bbai_last_error()
    assert lib.bbai_set_grid_target(h, ctypes.c_void_p(env.full.data_ptr()), 12) == ERR_ARG and b"tile size" in lib.bbai_last_error()
    assert lib.bbai_set_grid_target(h, ctypes.c_void_p(env.full.data_ptr()), 0) == ERR_ARG
    assert lib.bbai_step_grid_target(h, None, *env._step_out(), env._stream()) == ERR_ARG
    env.step(acts)
    assert torch.equal(env.full, whole(env, ts))
    # no target
    assert lib.bbai_set_grid_target(h, None, ts) == 0 and valid() == 0
    assert lib.bbai_render_grid_target(h, env._stream()) == ERR_STATE and b"no grid target" in lib.bbai_last_error() and valid() == 0
    assert lib.bbai_step_grid_target(h, ctypes.c_void_p(acts.data_ptr()), *env._step_out(), env._stream()) == ERR_STATE and valid() == 0
    # no atlas of the registered tile size
    assert lib.bbai_set_grid_target(h, ctypes.c_void_p(env.full.data_ptr()), 32) == 0        # (the buffer is too small for 32: nothing is drawn)
    assert lib.bbai_render_grid_target(h, env._stream()) == ERR_STATE and b"no atlas" in lib.bbai_last_error() and valid() == 0
    assert lib.bbai_set_grid_target(h, ctypes.c_void_p(env.full.data_ptr()), ts) == 0 and valid() == 0
    env.step(acts)
    assert valid() == 1 and torch.equal(env.full, whole(env, ts))
    # the shadow readback
    assert lib.bbai_grid_target_shadow(h, None, env._stream()) == ERR_ARG
    other = make_env(gpu, ROOM, n, ts, full_obs=False)
    out = torch.zeros((n, 64), dtype=torch.uint8, device=gpu)
    assert other.lib.bbai_grid_target_shadow(other.handle, ctypes.c_void_p(out.data_ptr()), other._stream()) == ERR_STATE
