"""The delta render's store unit (option "render_piece_bytes"): 64-byte pieces (the default) against whole 128-byte lines.  Every test steps
a handle with a piece size and one with 128 (the line rule) with the same actions and compares them byte for byte: pixels, encodings and
the registered buffer's tile ids (bbai_render_shadow) -- through both delta kernels: render_delta_from_step 1 (k_render_dstore) and 0
(k_render_delta).  At the end the pixels are also checked against a full render of the encoding into a buffer the handle does not own."""
import ctypes

import pytest

BOSS = "BabyAI-BossLevel-v0"
ROOM = "BabyAI-GoToLocal-v0"
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


def pair(gpu, n, piece, from_step, level=BOSS, seeds=11, **kw):
    from babyai_amd.engine import BatchedBabyAIEnv
    a = BatchedBabyAIEnv(level, n, device=gpu, pixel=True, seeds=seeds, **kw)
    _open.append(a)
    b = BatchedBabyAIEnv(level, n, device=gpu, pixel=True, seeds=seeds, **kw)
    _open.append(b)
    assert a.get_option("render_piece_bytes") == 64           # (the default)
    a.set_option("render_piece_bytes", piece)
    b.set_option("render_piece_bytes", 128)
    assert a.get_option("render_piece_bytes") == piece and b.get_option("render_piece_bytes") == 128
    for e in (a, b):
        e.set_option("render_delta_from_step", from_step)
    a.reset()
    b.reset()
    return a, b


def same(a, b):
    import torch
    return torch.equal(a.pixels, b.pixels) and torch.equal(a.image, b.image) and torch.equal(a.render_shadow(), b.render_shadow())


def full_render(env):
    import torch
    return env.render_encoding(out=torch.empty_like(env.pixels))


@pytest.mark.gpu
def test_option_values(gpu):
    from babyai_amd.engine import BatchedBabyAIEnv
    e = BatchedBabyAIEnv(ROOM, 64, device=gpu, pixel=True, seeds=3)
    _open.append(e)
    for v in (64, 128):
        e.set_option("render_piece_bytes", v)
        assert e.get_option("render_piece_bytes") == v
    for v in (0, 16, 32, 48, 256):
        with pytest.raises(Exception):
            e.set_option("render_piece_bytes", v)
    assert e.get_option("render_piece_bytes") == 128


@pytest.mark.gpu
@pytest.mark.parametrize("from_step", [1, 0])
@pytest.mark.parametrize("level,n", [(BOSS, 4096 + 5), (ROOM, 65536 + 64 + 3)])
def test_pieces_equal_lines(gpu, level, n, from_step):
    """Odd batch sizes (a partial last group); GoToLocal finishes about 2 % of its envs per random step, so resets are crossed."""
    import torch
    from babyai_amd.action_stream import actions_torch
    a, b = pair(gpu, n, 64, from_step, level=level, seeds=19)
    T = 120
    acts = actions_torch(3, 0, T, 0, n, gpu)
    done = 0
    for t in range(T):
        a.step(acts[t])
        b.step(acts[t])
        done += int(a.done.sum())
        if t % 10 == 0:
            assert same(a, b), t
    assert same(a, b) and done > 0
    assert a.get_option("render_delta_valid") == 1
    assert torch.equal(full_render(a), a.pixels)


@pytest.mark.gpu
@pytest.mark.parametrize("from_step", [1, 0])
def test_pieces_at_scale(gpu, from_step):
    import torch
    from babyai_amd.action_stream import actions_torch
    n = 1048576
    a, b = pair(gpu, n, 64, from_step)
    acts = actions_torch(4, 0, 40, 0, n, gpu)
    for t in range(40):
        a.step(acts[t])
        b.step(acts[t])
        if t % 13 == 0:
            assert same(a, b), t
    assert same(a, b)
    assert torch.equal(full_render(a), a.pixels)


@pytest.mark.gpu
@pytest.mark.parametrize("from_step", [1, 0])
def test_split_step_halves(gpu, from_step):
    """bbai_step_render in two halves: the second half's render starts at an env offset."""
    import torch
    from babyai_amd.action_stream import actions_torch
    n = 262144 + 64 + 5
    a, b = pair(gpu, n, 64, from_step, seeds=8)
    for e in (a, b):
        e.set_option("step_render_split", 1)
    acts = actions_torch(6, 0, 60, 0, n, gpu)
    for t in range(60):
        a.step(acts[t])
        b.step(acts[t])
        if t % 8 == 0:
            assert same(a, b), t
    assert same(a, b)
    assert torch.equal(full_render(a), a.pixels)


@pytest.mark.gpu
@pytest.mark.parametrize("from_step", [1, 0])
@pytest.mark.parametrize("split", [0, 1])
def test_rollout_with_pixel_taps(gpu, from_step, split):
    import torch
    from babyai_amd.action_stream import actions_torch
    from babyai_amd.shard import scattered_ids
    n, T, P, PP = 131072 + 3, 48, 64, 16
    a, b = pair(gpu, n, 64, from_step, seeds=13)
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
    assert torch.equal(full_render(a), a.pixels)


@pytest.mark.gpu
def test_bare_render_after_step(gpu):
    """bbai_step, then bbai_render into the registered buffer (k_render_delta), on both handles."""
    import torch
    from babyai_amd.action_stream import actions_torch
    n = 65536 + 7
    a, b = pair(gpu, n, 64, 0, seeds=29)
    acts = actions_torch(9, 0, 40, 0, n, gpu)
    for t in range(40):
        for e in (a, b):
            s = e._stream()
            assert e.lib.bbai_step(e.handle, ctypes.c_void_p(acts[t].data_ptr()), ctypes.c_void_p(e.image.data_ptr()), ctypes.c_void_p(e.direction.data_ptr()),
                                   ctypes.c_void_p(e.reward.data_ptr()), ctypes.c_void_p(e.reward64.data_ptr()), ctypes.c_void_p(e.done.data_ptr()), 1, s) == 0
            assert e.lib.bbai_render(e.handle, ctypes.c_void_p(e.image.data_ptr()), ctypes.c_void_p(e.pixels.data_ptr()), s) == 0
        if t % 5 == 0:
            assert same(a, b), t
    assert same(a, b)
    assert a.get_option("render_delta_valid") == 1
    assert torch.equal(full_render(a), a.pixels)
