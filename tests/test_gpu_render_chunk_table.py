"""The piece stores of the delta render address their 16-byte chunks through a per-block table (chunk_recipe / store_chunk16_t in
bbai_render.hpp) where the full renders (k_render / k_render_q) work the same geometry out per store.  After EVERY step of a short run the
registered pixel buffer -- written by the table form, k_render_dstore with the option "render_delta_from_step" at 1 and k_render_delta
with it at 0 -- must equal, byte for byte, a full render of the same encoding into a buffer the handle does not own.  The batch sizes:
one env; a full 32-env group plus one; several groups with a partial last one; and more than 3 x 256 x 32 envs, where a block loops over
more than one group and the last group is partial.  (The table itself is held against render_chunk's arithmetic by a static_assert that
the device build and the tests/hostsim build both compile.)"""
import pytest

BOSS = "BabyAI-BossLevel-v0"
STEPS = 30
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


def make(gpu, n, from_step):
    from babyai_amd.engine import BatchedBabyAIEnv
    env = BatchedBabyAIEnv(BOSS, n, device=gpu, pixel=True, seeds=31)       # (auto_reset: the default, on)
    _open.append(env)
    assert env.get_option("render_delta") == 1 and env.get_option("render_piece_bytes") == 64
    env.set_option("render_delta_from_step", from_step)
    assert env.get_option("render_delta_from_step") == from_step
    env.reset()
    return env


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 33, 97, 24609])
def test_table_stores_equal_the_full_render_after_every_step(gpu, n):
    import torch
    from babyai_amd.action_stream import actions_torch
    a, b = make(gpu, n, 1), make(gpu, n, 0)
    acts = actions_torch(12, 0, STEPS, 0, n, gpu)
    ref = torch.empty_like(a.pixels)                    # not registered: render_encoding renders it in full
    changed = 0
    for t in range(STEPS):
        before = a.pixels.clone()
        a.step(acts[t])
        b.step(acts[t])
        assert torch.equal(a.image, b.image), (n, t)
        a.render_encoding(out=ref)
        assert torch.equal(a.pixels, ref), ("k_render_dstore", n, t)
        assert torch.equal(b.pixels, ref), ("k_render_delta", n, t)
        assert torch.equal(a.render_shadow(), b.render_shadow()), (n, t)
        changed += int((before != a.pixels).any())
    assert a.get_option("render_delta_valid") == 1 and b.get_option("render_delta_valid") == 1      # (delta renders, not full ones)
    assert changed > 0                                  # the run did draw
