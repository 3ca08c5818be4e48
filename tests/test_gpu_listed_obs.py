"""The listed-env observation kernels (k_view_obs<V>, k_full_obs, k_render_grid<TS>) on an id list long enough that every persistent block
works SEVERAL items: the next item's entries are loaded under the current item's work (bbai_kernels.hpp list_item_load), the last item is
ragged, and ids outside [0, n) fall into first, middle and last items.  The other tests of these kernels list a few hundred envs: there
no block ever sees a second item.

A batch of 64 envs; the list has 2 B EPI + EPI + 7 entries with repeats, B = the launch's blocks (CUs x the family's blocks per CU) and
EPI = the family's envs per item -- every block gets two full items, the first blocks a third, the last item holds 7 envs.  Expected: the
frames of all 64 envs (which the families' own tests hold to the oracle) gathered by the list, zero frames for ids outside the batch;
compared byte for byte, with guard bytes on both sides of the output.  Both state layouts: the record resolver has two branches."""
import numpy as np
import pytest

LEVEL = "GoToLocalS5N2"
N = 64
GUARD = 256


def make(gpu, inplace, monkeypatch):
    from babyai_amd.engine import BatchedBabyAIEnv
    import torch
    monkeypatch.setenv("BBAI_INPLACE", inplace)
    env = BatchedBabyAIEnv("BabyAI-%s-v0" % LEVEL, N, device=gpu, seeds=77)
    assert env.get_option("inplace") == int(inplace)
    env.reset()
    rng = np.random.RandomState(3)
    for t in range(5):
        env.step(torch.as_tensor(rng.randint(0, 7, size=N).astype(np.uint8), device=gpu))
    return env


def id_list(gpu, blocks_per_cu, epi):
    """int64[2 B EPI + EPI + 7] over [-2, N + 2) from a seeded generator, some 1 << 40 among them; ids outside the batch in the first item,
    in the middle and in the last item for certain."""
    import torch
    blocks = torch.cuda.get_device_properties(gpu).multi_processor_count * blocks_per_cu
    count = 2 * blocks * epi + epi + 7
    ids = np.random.RandomState(11).randint(-2, N + 2, size=count).astype(np.int64)
    ids[[0, count // 2, count - 1]] = [-1, N, N + 1]
    ids[[3, count // 2 + 1, count - 2]] = 1 << 40
    assert count > 2 * blocks * epi and count % epi == 7
    return torch.as_tensor(ids, device=gpu)


def check(gpu, ids, frames_all, draw):
    """draw(ids, out) fills out[k] with the frame of env ids[k]; frames_all[i] is env i's."""
    import torch
    k, shape = ids.shape[0], tuple(frames_all.shape[1:])
    f = int(np.prod(shape))
    inside = (ids >= 0) & (ids < N)
    want = frames_all[ids.clamp(0, N - 1)] * inside.to(torch.uint8).reshape(-1, 1, 1, 1)
    assert not inside[0] and not inside[k // 2] and not inside[-1] and inside.sum() > k // 2
    buf = torch.zeros(GUARD + k * f + GUARD, dtype=torch.uint8, device=gpu)
    out = buf[GUARD:GUARD + k * f].view((k,) + shape)
    assert out.data_ptr() % 16 == 0
    got = draw(ids, out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out, want)
    assert not buf[:GUARD].any() and not buf[GUARD + k * f:].any()
    assert frames_all.any()


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", ["0", "1"])
@pytest.mark.parametrize("V,epi", [(3, 256), (11, 48)])            # bbai_viewn.hpp ViewN<V>::EPI: the largest and the smallest
def test_view_blocks_work_several_items(gpu, V, epi, inplace, monkeypatch):
    env = make(gpu, inplace, monkeypatch)
    ids = id_list(gpu, 4, epi)                                     # bbai_viewn.hpp VIEWN_BPC
    check(gpu, ids, env.observe_view(view_size=V), lambda i, o: env.observe_view(i, view_size=V, out=o))
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", ["0", "1"])
def test_full_blocks_work_several_items(gpu, inplace, monkeypatch):
    env = make(gpu, inplace, monkeypatch)
    c = env.cfg
    f = 3 * c.W * c.H
    align = 16 // int(np.gcd(f, 16))
    # bbai_engine.hip full_launch: FULL_MAX_ENVS, FULL_LDS / F, FULL_APP / (H ES) of bbai_gridk.hpp, a multiple of 16 / gcd(F, 16)
    epi = min(128, 24576 // f, 16384 // (c.H * c.ES)) // align * align
    assert epi >= 16
    ids = id_list(gpu, 3, epi)                                     # bbai_gridk.hpp FULL_BPC
    check(gpu, ids, env.observe_full(), lambda i, o: env.observe_full(i, out=o))
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", ["0", "1"])
def test_grid_blocks_work_several_items(gpu, inplace, monkeypatch):
    env = make(gpu, inplace, monkeypatch)
    c, ts = env.cfg, 8
    f = c.H * ts * c.W * ts * 3
    assert f <= 65536                                              # bbai_engine.hip render_grid_launch: small frames, several envs per item
    epi = max(1, min(131072 // f, 32, 4096 // (c.W * c.H)))        # ... 128 KB of frames, bbai_gridk.hpp GRID_MAX_ENVS, GRID_ID_BYTES / (W H)
    ids = id_list(gpu, 2, epi)                                     # ... two blocks per CU at tile size 8
    check(gpu, ids, env.render_grid(tile_size=ts), lambda i, o: env.render_grid(i, tile_size=ts, out=o))
    env.close()
