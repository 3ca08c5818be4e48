"""Dirty cells found by the step (option "render_delta_from_step"): a step + render call whose render is a delta render of the registered
target lets k_step find the changed tile ids and the dirty masks, and the render only stores (k_render_dstore).  The default, -1,
takes that path from 786 432 envs up.  Every test steps a handle with the option 1 and one with the option 0 (the render finds the dirty
cells itself, k_render_delta) with the same actions and compares them byte for byte: pixels, encodings and the registered buffer's tile ids (bbai_render_shadow); at the end the pixels also
against a full render of the encoding into a buffer the handle does not own."""
import ctypes

import numpy as np
import pytest

BOSS = "BabyAI-BossLevel-v0"
ROOM = "BabyAI-GoToLocal-v0"        # a single room: the in-place layout (look-ahead slots moved on inside k_step)
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


def pair(gpu, n, level=BOSS, seeds=11, **kw):
    from babyai_amd.engine import BatchedBabyAIEnv
    a = BatchedBabyAIEnv(level, n, device=gpu, pixel=True, seeds=seeds, **kw)
    _open.append(a)
    b = BatchedBabyAIEnv(level, n, device=gpu, pixel=True, seeds=seeds, **kw)
    _open.append(b)
    assert a.get_option("render_delta_from_step") == -1 and a.get_option("render_delta") == 1      # (default: by batch size)
    a.set_option("render_delta_from_step", 1)
    b.set_option("render_delta_from_step", 0)
    assert b.get_option("render_delta_from_step") == 0
    a.reset()
    b.reset()
    return a, b


def same(a, b):
    import torch
    return torch.equal(a.pixels, b.pixels) and torch.equal(a.image, b.image) and torch.equal(a.render_shadow(), b.render_shadow())


def full_render(env):
    import torch
    return env.render_encoding(out=torch.empty_like(env.pixels))


def boss_actions(env, acts, t):
    import torch
    if acts is not None:
        return acts[t]
    act = env.bot_actions()
    return torch.where(act > 6, torch.full_like(act, 6), act)       # (a bot that gave up: the done action)


@pytest.mark.gpu
@pytest.mark.parametrize("n,T,every", [(1024, 200, 1), (131072, 150, 10), (1048576, 60, 20)])
@pytest.mark.parametrize("policy", ["random", "expert"])
def test_from_step_equals_render_side(gpu, n, T, every, policy):
    import torch
    from babyai_amd.action_stream import actions_torch
    a, b = pair(gpu, n)
    acts = actions_torch(3, 0, T, 0, n, gpu) if policy == "random" else None
    for t in range(T):
        act = boss_actions(a, acts, t)
        a.step(act)
        b.step(act)
        if t % every == 0 or t == T - 1:
            assert same(a, b), (n, policy, t)
    assert a.get_option("render_delta_valid") == 1
    assert torch.equal(full_render(a), a.pixels)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1024 + 5, 65536 + 64 + 3])
def test_single_room_in_place_with_resets(gpu, n):
    """GoToLocal: about 2 % of the envs finish on every random step and move on inside k_step; the odd batch size ends in a partial block."""
    import torch
    from babyai_amd.action_stream import actions_torch
    a, b = pair(gpu, n, level=ROOM, seeds=23)
    acts = actions_torch(5, 0, 200, 0, n, gpu)
    done = 0
    for t in range(200):
        a.step(acts[t])
        b.step(acts[t])
        done += int(a.done.sum())
        if t % 10 == 0:
            assert same(a, b), t
    assert same(a, b) and done > 0
    assert torch.equal(full_render(a), a.pixels)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [ROOM, BOSS])
def test_frozen_envs_without_auto_reset(gpu, level):
    """auto_reset=False: k_step finds the dirty cells of a step whose finished envs freeze and re-emit their last observation (the branch of
    bbai_step_render for `!auto_reset`), in the in-place layout (GoToLocal) and the classic one (BossLevel), at an odd batch size past the
    option's default threshold; reset commands (action 7) freeze envs of both levels, a reset() in mid-run thaws them all."""
    import torch
    from babyai_amd.action_stream import actions_torch
    n, T = 786432 + 64 + 3, 60
    a, b = pair(gpu, n, level=level, seeds=29, auto_reset=False)
    assert a.get_option("inplace") == (1 if level == ROOM else 0)
    acts = actions_torch(9, 0, T, 0, n, gpu)
    gen = torch.Generator(device=gpu)
    gen.manual_seed(4)
    frozen = 0
    for t in range(T):
        if t == 40:
            a.reset()
            b.reset()
            assert same(a, b), t
        act = torch.where(torch.rand((n,), device=gpu, generator=gen) < 0.01, torch.full_like(acts[t], 7), acts[t])
        a.step(act)
        b.step(act)
        if t == 39:
            frozen = int(a.done.sum())
        if t % 10 == 0 or t == 39:
            assert same(a, b), t
    assert same(a, b) and frozen > n // 5
    assert torch.equal(a.done, b.done) and torch.equal(a.reward64, b.reward64)
    assert torch.equal(full_render(a), a.pixels)


@pytest.mark.gpu
@pytest.mark.parametrize("split", [0, 1])
def test_split_steps(gpu, split):
    """bbai_step_render in two halves: both halves' renders take the step's dirty cells (the second one at an env offset)."""
    from babyai_amd.action_stream import actions_torch
    n = 262144 + 64 + 5
    a, b = pair(gpu, n, seeds=8)
    for e in (a, b):
        e.set_option("step_render_split", split)
    acts = actions_torch(6, 0, 60, 0, n, gpu)
    for t in range(60):
        a.step(acts[t])
        b.step(acts[t])
        if t % 8 == 0:
            assert same(a, b), t
    assert same(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [BOSS, ROOM])
@pytest.mark.parametrize("split", [0, 1])
def test_rollout_with_pixel_taps(gpu, level, split):
    import torch
    from babyai_amd.action_stream import actions_torch
    from babyai_amd.shard import scattered_ids
    n, T, P, PP = 131072 + 3, 48, 64, 16
    a, b = pair(gpu, n, level=level, seeds=13)
    for e in (a, b):
        e.set_option("step_render_split", split)
    ids = torch.as_tensor(scattered_ids(n, P), dtype=torch.int64, device=gpu)

    def mklog():
        return {"image": torch.zeros((T + 1, P, 7, 7, 3), dtype=torch.uint8, device=gpu), "direction": torch.zeros((T + 1, P), dtype=torch.uint8, device=gpu),
                "reward64": torch.zeros((T, P), dtype=torch.float64, device=gpu), "done": torch.zeros((T, P), dtype=torch.uint8, device=gpu), "ids": ids,
                "pixels": torch.zeros((T + 1, PP, 56, 56, 3), dtype=torch.uint8, device=gpu)}
    la, lb = mklog(), mklog()
    acts = actions_torch(7, 0, T, 0, n, gpu)
    for k in range(0, T, 16):
        a.rollout(acts[k:k + 16], tap=la, obs_row0=k + 1, row0=k)
        b.rollout(acts[k:k + 16], tap=lb, obs_row0=k + 1, row0=k)
        assert same(a, b), k
    for key in la:
        assert torch.equal(la[key], lb[key]), key


@pytest.mark.gpu
def test_history_events_between_steps(gpu):
    """render_invalidate, a checkpoint load, reset() and an atlas re-install between steps, and the option switched mid-run."""
    import torch
    from babyai_amd.action_stream import actions_torch
    from babyai_amd.engine import ATLAS_PATH
    n = 4096 + 8 + 1
    a, b = pair(gpu, n, seeds=17)
    acts = actions_torch(8, 0, 200, 0, n, gpu)
    t = 0

    def run(k):
        nonlocal t
        for _ in range(k):
            a.step(acts[t])
            b.step(acts[t])
            assert same(a, b), t
            t += 1
    run(15)
    a.pixels[::3].fill_(0x5A)
    a.render_invalidate()
    b.pixels[::3].fill_(0x5A)
    b.render_invalidate()
    run(10)
    blob_a, blob_b = a.save_checkpoint(), b.save_checkpoint()
    run(15)
    a.load_checkpoint(blob_a)
    b.load_checkpoint(blob_b)
    run(10)
    a.reset()
    b.reset()
    run(10)
    atlas = np.load(ATLAS_PATH)
    tiles = np.ascontiguousarray(atlas["tiles"], dtype=np.uint8)
    lut = np.ascontiguousarray(atlas["lut"], dtype=np.uint8)
    alt = np.ascontiguousarray(255 - tiles)
    for e in (a, b):
        assert e.lib.bbai_set_atlas(e.handle, alt.ctypes.data, alt.shape[0], lut.ctypes.data) == 0
    run(10)
    for e in (a, b):
        assert e.lib.bbai_set_atlas(e.handle, tiles.ctypes.data, tiles.shape[0], lut.ctypes.data) == 0
    run(10)
    a.set_option("render_delta_from_step", 0)
    run(5)
    a.set_option("render_delta_from_step", 1)
    run(10)
    a.set_option("render_delta_from_step", -1)      # (4 105 envs: by batch size, the render-side path)
    assert a.get_option("render_delta_from_step") == -1
    run(5)
    assert torch.equal(full_render(a), a.pixels)


@pytest.mark.gpu
def test_step_then_render_and_unfused_consume(gpu):
    """A bare bbai_step + bbai_render pair keeps the render-side path; so does a step whose finished envs are consumed by a later launch."""
    import torch
    from babyai_amd.action_stream import actions_torch
    n = 65536 + 7
    a, b = pair(gpu, n, seeds=29)
    acts = actions_torch(9, 0, 90, 0, n, gpu)
    s = a._stream()
    for t in range(30):
        assert a.lib.bbai_step(a.handle, ctypes.c_void_p(acts[t].data_ptr()), ctypes.c_void_p(a.image.data_ptr()), ctypes.c_void_p(a.direction.data_ptr()),
                               ctypes.c_void_p(a.reward.data_ptr()), ctypes.c_void_p(a.reward64.data_ptr()), ctypes.c_void_p(a.done.data_ptr()), 1, s) == 0
        assert a.lib.bbai_render(a.handle, ctypes.c_void_p(a.image.data_ptr()), ctypes.c_void_p(a.pixels.data_ptr()), s) == 0
        b.step(acts[t])
        assert same(a, b), t
    for e in (a, b):
        e.set_option("consume_fused", 0)
    for t in range(30, 60):
        a.step(acts[t])
        b.step(acts[t])
        assert same(a, b), t
    for e in (a, b):
        e.set_option("consume_fused", -1)
    for t in range(60, 90):
        a.step(acts[t])
        b.step(acts[t])
    assert same(a, b)
    assert torch.equal(full_render(a), a.pixels)
