"""step_dirty (the dirty scan at the tail of k_step, four cells per word: babyai_amd/csrc/bbai_dirty.hpp) at the smallest batches at which
it can go wrong, by the pair method of tests/test_gpu_render_delta_from_step.py: a handle with option "render_delta_from_step" 1 (k_step
finds the dirty cells, the render only stores) against one with the option 0 (the render finds them itself), the same actions, and pixels,
encodings and the registered buffer's tile ids (render_shadow) compared byte for byte after EVERY step.  Sizes: 1 env (49 shadow bytes =
three chunks and a one-byte tail), 2 and 21, 63 / 64 / 65 and 85 around the 64-env block, 64 x 3 + 1 (three full blocks and a one-env
one).  Random and expert steps on BossLevel (the expert's pickups and drops change the agent's cell, the one id of the second table), random
steps across auto-resets on GoToLocal (the in-place layout), a run without auto-reset in which frozen lanes re-emit their rows, and a run
on an installed lut whose agent's half differs from the plain half on every key while several keys share an id."""
import numpy as np
import pytest

BOSS = "BabyAI-BossLevel-v0"        # the classic layout; the stepping wave consumes its finished envs (option consume_fused 1)
ROOM = "BabyAI-GoToLocal-v0"        # a single room: the in-place layout
SIZES = [1, 2, 21, 63, 64, 65, 85, 64 * 3 + 1]
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
    envs = []
    for option in (1, 0):
        e = BatchedBabyAIEnv(level, n, device=gpu, pixel=True, seeds=seeds, **kw)
        _open.append(e)
        if level == BOSS:
            e.set_option("consume_fused", 1)            # (k_step's rows are then the step's final observations at every batch size)
        else:
            assert e.get_option("inplace") == 1
        e.set_option("render_delta_from_step", option)
        assert e.get_option("render_delta_from_step") == option and e.get_option("render_delta") == 1
        envs.append(e)
    for e in envs:
        e.reset()
    return envs


def same(a, b):
    import torch
    return torch.equal(a.pixels, b.pixels) and torch.equal(a.image, b.image) and torch.equal(a.render_shadow(), b.render_shadow())


def full_render(env):
    import torch
    return env.render_encoding(out=torch.empty_like(env.pixels))


def expert_actions(env):
    import torch
    act = env.bot_actions()
    return torch.where(act > 6, torch.full_like(act, 6), act)       # (a bot that gave up: the done action)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_boss_random_then_expert(gpu, n):
    import torch
    from babyai_amd.action_stream import actions_torch
    a, b = pair(gpu, n)
    carried = 0
    for t in range(60):                                  # (the expert first: it plans from the reset on)
        act = expert_actions(a)
        a.step(act)
        b.step(act)
        assert same(a, b), (n, "expert", t)
        carried += int((act == 3).sum()) + int((act == 4).sum())
    assert n < 64 or carried > 0, "no pickup or drop in 60 expert steps: the agent's cell never changed"
    acts = actions_torch(3, 0, 120, 0, n, gpu)
    for t in range(120):
        a.step(acts[t])
        b.step(acts[t])
        assert same(a, b), (n, "random", t)
    assert a.get_option("render_delta_valid") == 1
    assert torch.equal(full_render(a), a.pixels)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_room_in_place_with_auto_resets(gpu, n):
    import torch
    from babyai_amd.action_stream import actions_torch
    a, b = pair(gpu, n, level=ROOM, seeds=23)
    acts = actions_torch(5, 0, 120, 0, n, gpu)
    done = 0
    for t in range(120):
        a.step(acts[t])
        b.step(acts[t])
        done += int(a.done.sum())
        assert same(a, b), (n, t)
    assert n < 21 or done > 0
    assert torch.equal(full_render(a), a.pixels)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [BOSS, ROOM])
def test_frozen_lanes_re_emit_their_rows(gpu, level):
    """auto_reset=False: reset commands (action 7) and finished episodes freeze envs, whose rows are copied through LDS unchanged -- a block
    then mixes stepping and frozen lanes; a reset() in mid-run thaws them all."""
    import torch
    from babyai_amd.action_stream import actions_torch
    n, T = 64 * 3 + 1, 90
    a, b = pair(gpu, n, level=level, seeds=29, auto_reset=False)
    acts = actions_torch(9, 0, T, 0, n, gpu)
    gen = torch.Generator(device=gpu)
    gen.manual_seed(4)
    frozen = 0
    for t in range(T):
        if t == 50:
            a.reset()
            b.reset()
            assert same(a, b), t
        act = torch.where(torch.rand((n,), device=gpu, generator=gen) < 0.02, torch.full_like(acts[t], 7), acts[t])
        a.step(act)
        b.step(act)
        if t == 49:
            frozen = int(a.done.sum())
        assert same(a, b), (level, t)
    assert 0 < frozen < n, frozen          # (blocks with stepping AND frozen lanes)
    assert torch.equal(a.done, b.done) and torch.equal(a.reward64, b.reward64)
    assert torch.equal(full_render(a), a.pixels)


@pytest.mark.gpu
def test_installed_lut_agent_half_differs_and_keys_share_ids(gpu):
    """A lut installed with bbai_set_atlas: plain half = key % 5 (several keys share an id: a changed encoding with an unchanged id is not
    dirty), agent's half = 5 + key % 3 (differs from the plain half on EVERY key, so the second table shows in the shadow at cell 27 of
    every env on every step)."""
    import torch
    from babyai_amd.action_stream import actions_torch
    from babyai_amd.engine import ATLAS_PATH
    n = 85
    a, b = pair(gpu, n, seeds=17)
    atlas = np.load(ATLAS_PATH)
    tiles = np.ascontiguousarray(atlas["tiles"], dtype=np.uint8)
    assert tiles.shape[0] >= 8
    key = np.arange(256)
    lut = np.ascontiguousarray(np.stack([key % 5, 5 + key % 3]), dtype=np.uint8)
    assert (lut[0] != lut[1]).all() and len(set(lut[0].tolist())) < 256
    for e in (a, b):
        assert e.lib.bbai_set_atlas(e.handle, tiles.ctypes.data, tiles.shape[0], lut.ctypes.data) == 0
    acts = actions_torch(8, 0, 80, 0, n, gpu)
    for t in range(120):
        act = expert_actions(a) if t < 40 else acts[t - 40]
        a.step(act)
        b.step(act)
        assert same(a, b), t
    shadow = a.render_shadow().cpu().numpy()
    enc = a.image.cpu().numpy().reshape(n, 49, 3).astype(np.int64)
    keys = enc[:, :, 0] | enc[:, :, 1] << 3 | enc[:, :, 2] << 6
    want = lut[0][keys]
    want[:, 27] = lut[1][keys[:, 27]]
    assert np.array_equal(shadow, want)
    assert (shadow[:, 27] >= 5).all() and (np.delete(shadow, 27, axis=1) < 5).all()
    assert torch.equal(full_render(a), a.pixels)
