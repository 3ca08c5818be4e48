"""The agent's 7x7 view as pixels at tile sizes 16 and 32 on the device (k_view_pixels, include/bbai.h bbai_render_view): byte for byte
against the oracle's RGBImgPartialObsWrapper(env, tile_size) of envs driven the same way, every lut entry against a numpy gather of the
atlas, the launch's edge shapes, rollouts, the adapters, and never a byte outside the frames asked for."""
import numpy as np
import pytest

from test_gpu_parity import _oracle_envs
from test_view_atlas import load_atlas, view_frames

TS = (16, 32)
ACTIONS = np.array([0, 1, 2, 2, 2, 2, 3, 3, 5, 5, 4, 6], dtype=np.uint8)      # biased towards forward / pickup / toggle


def _wrappers(refs, ts):
    from oracle import refenv
    refenv.enable_shim()
    from gym_minigrid.wrappers import RGBImgPartialObsWrapper
    return [RGBImgPartialObsWrapper(r, tile_size=ts) for r in refs]


@pytest.mark.gpu
@pytest.mark.parametrize("ts", TS)
@pytest.mark.parametrize("level", ["GoToLocal", "BossLevel", "PutNextS5N2Carrying", "KeyCorridorS3R1"])
def test_live_frames_match_the_oracle_wrapper(gpu, level, ts):
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    n, steps, seed = 8, 48, 300
    env = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device=gpu, seeds=seed, pixel=True, tile_size=ts)
    assert tuple(env.pixels.shape) == (n, 7 * ts, 7 * ts, 3)
    refs = _oracle_envs(level, [seed + i for i in range(n)])
    wraps = _wrappers(refs, ts)
    obs_ref = [r.reset() for r in refs]
    obs = env.reset()
    rng = np.random.RandomState(ts)
    for t in range(steps + 1):
        assert obs["image"] is env.pixels
        pix = obs["image"].cpu().numpy()
        for i in range(n):
            want = wraps[i].observation(obs_ref[i])["image"]
            assert np.array_equal(pix[i], want), (level, ts, t, i, np.argwhere(pix[i] != want)[:4].tolist())
        if t == steps:
            break
        a = ACTIONS[rng.randint(0, len(ACTIONS), size=n)]
        obs, _, done, _ = env.step(torch.as_tensor(a, device=gpu))
        dn = done.cpu().numpy()
        for i in range(n):
            o, _, d, _ = refs[i].step(int(a[i]))
            assert bool(d) == bool(dn[i]), (t, i)
            obs_ref[i] = refs[i].reset() if d else o
    env.close()


def _every_key_batch():
    """uint8[512, 7, 7, 3]: every cell runs through all 256 keys (twice, in two orders) -- keys no object has and the agent's cell included."""
    r = np.arange(512)[:, None]
    c = np.arange(49)[None, :]
    key = np.where(r < 256, r + 37 * c, r + 101 * c + 13) % 256
    for cell in range(49):
        assert len(set(key[:, cell].tolist())) == 256
    return np.stack([key & 7, (key >> 3) & 7, key >> 6], axis=-1).astype(np.uint8).reshape(512, 7, 7, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("ts", TS)
def test_every_lut_entry_of_every_cell(gpu, ts):
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    env = BatchedBabyAIEnv("BabyAI-GoToLocal-v0", 8, device=gpu, seeds=1)
    enc = _every_key_batch()
    got = env.render_encoding(torch.as_tensor(enc, device=gpu), tile_size=ts)
    assert tuple(got.shape) == (512, 7 * ts, 7 * ts, 3)
    want = view_frames(enc, *load_atlas(ts), ts)
    assert np.array_equal(got.cpu().numpy(), want)
    env.close()


@pytest.fixture(scope="module")
def wide_batch(gpu):
    """1025 GoToLocal envs a few steps in, and the frames a numpy gather of the atlas makes of their encodings (computed once per tile size)."""
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    n = 1025
    env = BatchedBabyAIEnv("BabyAI-GoToLocal-v0", n, device=gpu, seeds=4000)
    env.reset()
    rng = np.random.RandomState(5)
    for t in range(6):
        env.step(torch.as_tensor(ACTIONS[rng.randint(0, len(ACTIONS), size=n)], device=gpu))
    enc = env.image.cpu().numpy()
    want = {}

    def frames(ts):
        if ts not in want:
            want[ts] = view_frames(enc, *load_atlas(ts), ts)
        return want[ts]
    yield env, frames
    env.close()


def _render_guarded(env, ids, ts, count):
    """render_view into a buffer one frame longer than asked, pre-filled with 0xAB: (frames, the extra frame)."""
    import torch
    buf = torch.full((count + 1, 7 * ts, 7 * ts, 3), 0xAB, dtype=torch.uint8, device=env.device)
    out = env.render_view(ids, tile_size=ts, out=buf[:count])
    assert out.data_ptr() == buf.data_ptr()
    return buf[:count].cpu().numpy(), buf[count].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("ts", TS)
@pytest.mark.parametrize("count", [1, 2, 3, 5, 33, 97, 1025])
def test_edge_counts(gpu, wide_batch, ts, count):
    env, frames = wide_batch
    want = frames(ts)
    got, guard = _render_guarded(env, list(range(count)), ts, count)
    assert np.array_equal(got, want[:count])
    assert (guard == 0xAB).all()
    if count == env.num_envs:
        got, guard = _render_guarded(env, None, ts, count)          # ids=None = arange
        assert np.array_equal(got, want)
        assert (guard == 0xAB).all()


@pytest.mark.gpu
@pytest.mark.parametrize("ts", TS)
def test_id_lists(gpu, wide_batch, ts):
    import torch
    env, frames = wide_batch
    want = frames(ts)
    n = env.num_envs
    ids = [5, 5, 1024, 3, 5, 0, -1, n, 700, 1024, n + 7, -(2 ** 40)] + list(range(40, 19, -1))
    got, guard = _render_guarded(env, ids, ts, len(ids))
    for k, i in enumerate(ids):
        if 0 <= i < n:
            assert np.array_equal(got[k], want[i]), (k, i)
        else:
            assert not got[k].any(), (k, i)
    assert (guard == 0xAB).all()
    dev_ids = torch.arange(n - 1, -1, -1, device=gpu, dtype=torch.int64)                 # a device tensor, reversed
    assert np.array_equal(env.render_view(dev_ids, tile_size=ts).cpu().numpy(), want[::-1])
    assert tuple(env.render_view([], tile_size=ts).shape) == (0, 7 * ts, 7 * ts, 3)


@pytest.mark.gpu
def test_rollout_leaves_what_single_steps_leave(gpu):
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    n, T, ts = 96, 40, 16
    a = torch.as_tensor(ACTIONS[np.random.RandomState(9).randint(0, len(ACTIONS), size=(T, n))], device=gpu)
    one = BatchedBabyAIEnv("BabyAI-PickupLoc-v0", n, device=gpu, seeds=77, pixel=True, tile_size=ts)
    two = BatchedBabyAIEnv("BabyAI-PickupLoc-v0", n, device=gpu, seeds=77, pixel=True, tile_size=ts)
    one.reset()
    two.reset()
    for t in range(T):
        one.step(a[t])
    obs = two.rollout(a)
    assert obs["image"] is two.pixels
    for name in ("pixels", "image", "reward", "done", "direction"):
        assert torch.equal(getattr(one, name), getattr(two, name)), name
    assert np.array_equal(two.pixels.cpu().numpy(), view_frames(two.image.cpu().numpy(), *load_atlas(ts), ts))
    tap = {"pixels": torch.zeros((T, 4, 112, 112, 3), dtype=torch.uint8, device=gpu), "done": torch.zeros((T, 4), dtype=torch.uint8, device=gpu)}
    with pytest.raises(ValueError):
        two.rollout(a, tap=tap)
    one.close()
    two.close()


@pytest.mark.gpu
def test_adapters_hand_out_the_wrappers_images(gpu):
    from babyai_amd import vec_env
    level, n, seed = "GoToLocal", 4, 900
    for ts, single in ((16, False), (32, True)):
        m = 1 if single else n
        refs = _oracle_envs(level, [seed + i for i in range(m)])
        wraps = _wrappers(refs, ts)
        if single:
            v = vec_env.SingleEnv("BabyAI-%s-v0" % level, device=gpu, pixel=True, seed=seed, tile_size=ts)
        else:
            v = vec_env.BatchedParallelEnv("BabyAI-%s-v0" % level, n, device=gpu, pixel=True, seeds=[seed + i for i in range(n)], tile_size=ts)
        assert v.observation_space["image"].shape == (7 * ts, 7 * ts, 3)
        obs_ref = [r.reset() for r in refs]
        obs = v.reset()
        obs = [obs] if single else obs
        rng = np.random.RandomState(3)
        for t in range(13):
            for i in range(m):
                want = wraps[i].observation(obs_ref[i])
                assert sorted(obs[i].keys()) == ["image", "mission"]
                assert obs[i]["image"].shape == (7 * ts, 7 * ts, 3) and np.array_equal(obs[i]["image"], want["image"]), (ts, t, i)
                assert obs[i]["mission"] == want["mission"]
            a = [int(x) for x in ACTIONS[rng.randint(0, len(ACTIONS), size=m)]]
            if single:
                o, _, d, _ = v.step(a[0])
                obs, done = [o], [d]
            else:
                obs, _, done, _ = v.step(a)
            for i in range(m):
                o, _, d, _ = refs[i].step(a[i])
                assert bool(d) == bool(done[i])
                if d and single:
                    return v.close()          # (ManyEnvs protocol of a batch of one: the episode is over)
                obs_ref[i] = refs[i].reset() if d else o
        v.close()


@pytest.mark.gpu
def test_render_view_at_8_on_an_encoded_batch(gpu):
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    n = 64
    enc = BatchedBabyAIEnv("BabyAI-BossLevel-v0", n, device=gpu, seeds=11)
    pix = BatchedBabyAIEnv("BabyAI-BossLevel-v0", n, device=gpu, seeds=11, pixel=True)
    enc.reset()
    pix.reset()
    a = torch.as_tensor(ACTIONS[np.random.RandomState(2).randint(0, len(ACTIONS), size=(5, n))], device=gpu)
    for t in range(5):
        enc.step(a[t])
        pix.step(a[t])
    assert torch.equal(enc.image, pix.image)
    want = pix.render_encoding(out=torch.empty((n, 56, 56, 3), dtype=torch.uint8, device=gpu))
    assert torch.equal(enc.render_view(tile_size=8), want)
    ids = [3, 3, 63, -1, 0, n]
    got = enc.render_view(ids, tile_size=8)
    for k, i in enumerate(ids):
        assert torch.equal(got[k], want[i] if 0 <= i < n else torch.zeros_like(got[k])), (k, i)
    for ts in TS:          # ... and the larger sizes from the same encoded batch
        assert np.array_equal(enc.render_view(tile_size=ts).cpu().numpy(), view_frames(enc.image.cpu().numpy(), *load_atlas(ts), ts))
    enc.close()
    pix.close()


@pytest.mark.gpu
def test_entry_point_error_codes(gpu):
    import ctypes
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    env = BatchedBabyAIEnv("BabyAI-GoToLocal-v0", 4, device=gpu, seeds=1)
    env.reset()
    lib, h = env.lib, env.handle
    out = torch.zeros((4 * 150528 + 16,), dtype=torch.uint8, device=gpu)
    img, o = env.image.data_ptr(), out.data_ptr()
    assert lib.bbai_render_view(h, 32, img, 4, None, 4, o, None) == -3                 # no atlas of that size yet
    tiles, lut = load_atlas(32)
    tiles, lut = np.ascontiguousarray(tiles), np.ascontiguousarray(lut)
    assert lib.bbai_set_view_atlas(h, 8, tiles.ctypes.data, 58, lut.ctypes.data) == -1
    assert lib.bbai_set_view_atlas(h, 32, tiles.ctypes.data, 0, lut.ctypes.data) == -1
    assert lib.bbai_set_view_atlas(h, 32, tiles.ctypes.data, 65, lut.ctypes.data) == -1
    assert lib.bbai_set_view_atlas(h, 32, tiles.ctypes.data, 57, lut.ctypes.data) == -1      # a lut entry names tile 57
    assert lib.bbai_render_view(h, 32, img, 4, None, 4, o, None) == -3
    assert lib.bbai_set_view_atlas(h, 32, tiles.ctypes.data, 58, lut.ctypes.data) == 0
    assert lib.bbai_render_view(h, 16, img, 4, None, 4, o, None) == -3                 # (each size has its own)
    assert lib.bbai_render_view(h, 8, img, 4, None, 4, o, None) == -1
    assert lib.bbai_render_view(h, 32, img, 4, None, -1, o, None) == -1
    assert lib.bbai_render_view(h, 32, img, 4, None, 5, o, None) == -1                  # count > rows without ids
    assert lib.bbai_render_view(h, 32, img, 4, None, 4, None, None) == -1
    assert lib.bbai_render_view(h, 32, img, 4, None, 4, o + 8, None) == -1              # misaligned
    assert lib.bbai_render_view(h, 32, img, 4, None, 0, None, None) == 0
    assert lib.bbai_render_view(h, 32, img, 4, None, 4, o, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out[:4 * 150528].cpu().numpy().reshape(4, 224, 224, 3), view_frames(env.image.cpu().numpy(), tiles, lut, 32))
    assert not out[4 * 150528:].any()
    env.close()
