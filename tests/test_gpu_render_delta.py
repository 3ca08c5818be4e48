"""Delta rendering into the registered observation buffer (include/bbai.h bbai_set_render_target): the render stores only the
128-byte lines whose cells changed since the frame the buffer holds.  Every test compares the delta path byte for byte with full
renders -- a handle with option "render_delta" 0 stepped with the same actions, or a full render of the same encoding into a
buffer that is not registered."""
import ctypes

import numpy as np
import pytest

LEVEL = "BabyAI-BossLevel-v0"
_open = []


@pytest.fixture(autouse=True)
def _close_handles():
    """Each batch sizes its look-ahead ring from the free memory: hand every test's memory back before the next one."""
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


def pair(gpu, n, seeds=11, **kw):
    from babyai_amd.engine import BatchedBabyAIEnv
    a = BatchedBabyAIEnv(LEVEL, n, device=gpu, pixel=True, seeds=seeds, **kw)
    _open.append(a)
    b = BatchedBabyAIEnv(LEVEL, n, device=gpu, pixel=True, seeds=seeds, **kw)
    _open.append(b)
    b.set_option("render_delta", 0)
    assert a.get_option("render_delta") == 1
    a.reset()
    b.reset()
    return a, b


def same(a, b):
    import torch
    return torch.equal(a.pixels, b.pixels) and torch.equal(a.image, b.image)


def full_render(env):
    """The current encoding rendered in full into a buffer the handle does not own."""
    import torch
    return env.render_encoding(out=torch.empty_like(env.pixels))


@pytest.mark.gpu
@pytest.mark.parametrize("n,T,every", [(1024, 300, 1), (131072, 300, 10), (1048576, 200, 25)])
@pytest.mark.parametrize("policy", ["random", "expert"])
def test_delta_equals_full_render(gpu, n, T, every, policy):
    import torch
    from babyai_amd.action_stream import actions_torch
    a, b = pair(gpu, n)
    acts = actions_torch(3, 0, T, 0, n, gpu) if policy == "random" else None
    for t in range(T):
        act = acts[t] if acts is not None else a.bot_actions()
        if acts is None:
            act = torch.where(act > 6, torch.full_like(act, 6), act)       # (a bot that gave up: the done action)
        a.step(act)
        b.step(act)
        if t % every == 0 or t == T - 1:
            assert same(a, b), (n, policy, t)
    assert a.get_option("render_delta_valid") == 1
    assert torch.equal(full_render(a), a.pixels)


@pytest.mark.gpu
def test_delta_under_every_render_queue_shape(gpu):
    """The full-render shapes (render_queue 0 .. 11) still render whatever is not the registered target, byte for byte."""
    from babyai_amd.action_stream import actions_torch
    n = 262144 + 64 + 5
    a, b = pair(gpu, n, seeds=5)
    acts = actions_torch(4, 0, 12 * 24, 0, n, gpu)
    t = 0
    for qm in range(12):
        a.set_option("render_queue", qm)
        b.set_option("render_queue", qm)
        for _ in range(24):
            a.step(acts[t])
            b.step(acts[t])
            t += 1
        assert same(a, b), qm


@pytest.mark.gpu
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("sched,tpb", [(0, 512), (1, 512), (0, 1024)])
def test_delta_split_and_schedules(gpu, split, sched, tpb):
    """bbai_step_render split into halves (the second half renders at an env offset) and every delta work split."""
    from babyai_amd.action_stream import actions_torch
    n = 262144 + 64 + 5
    a, b = pair(gpu, n, seeds=8)
    a.set_option("step_render_split", split)
    a.set_option("render_delta_sched", sched)
    a.set_option("render_delta_tpb", tpb)
    acts = actions_torch(6, 0, 120, 0, n, gpu)
    for t in range(120):
        a.step(acts[t])
        b.step(acts[t])
        if t % 8 == 0:
            assert same(a, b), t
    assert same(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("split", [0, 1])
def test_delta_rollout_with_pixel_taps(gpu, split):
    import torch
    from babyai_amd.action_stream import actions_torch
    from babyai_amd.shard import scattered_ids
    n, T, P, PP = 131072 + 3, 64, 64, 16
    a, b = pair(gpu, n, seeds=13)
    a.set_option("step_render_split", split)
    b.set_option("step_render_split", split)
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
def test_delta_history_events(gpu):
    """What the registered history must survive or notice: a caller scribbling into the buffer (then invalidating), a render of the
    encoding into another buffer, reset(), a checkpoint load, an atlas re-install (the first render after it is a full one)."""
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
    run(20)
    a.pixels[::3].fill_(0x5A)                 # a caller writes into the registered buffer ...
    a.render_invalidate()                     # ... and says so
    assert a.get_option("render_delta_valid") == 0
    run(10)
    other = torch.empty_like(a.pixels)
    a.render_encoding(out=other)              # a render elsewhere leaves the history alone
    assert torch.equal(other, a.pixels) and a.get_option("render_delta_valid") == 1
    run(10)
    blob_a, blob_b = a.save_checkpoint(), b.save_checkpoint()
    run(15)
    a.load_checkpoint(blob_a)
    b.load_checkpoint(blob_b)
    run(10)
    oa, ob = a.reset(), b.reset()
    assert same(a, b)
    run(10)
    atlas = np.load(ATLAS_PATH)
    tiles = np.ascontiguousarray(atlas["tiles"], dtype=np.uint8)
    lut = np.ascontiguousarray(atlas["lut"], dtype=np.uint8)
    alt = np.ascontiguousarray(255 - tiles)
    for e in (a, b):
        assert e.lib.bbai_set_atlas(e.handle, alt.ctypes.data, alt.shape[0], lut.ctypes.data) == 0
    assert a.get_option("render_delta_valid") == 0
    run(10)
    for e in (a, b):
        assert e.lib.bbai_set_atlas(e.handle, tiles.ctypes.data, tiles.shape[0], lut.ctypes.data) == 0
    run(10)
    a.set_option("render_delta", 0)           # switching it off and on again: a full render first
    run(3)
    a.set_option("render_delta", 1)
    run(10)


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 16])
def test_delta_registered_buffer_alignment(gpu, offset):
    """A registered buffer 16 bytes off the 128-byte grid gets full renders (and the same bytes); an aligned one gets delta renders."""
    import torch
    from babyai_amd.action_stream import actions_torch
    n = 131072 + 5
    a, b = pair(gpu, n, seeds=19)
    raw = torch.zeros(n * 9408 + 256, dtype=torch.uint8, device=gpu)
    base = (-raw.data_ptr()) % 128 + offset
    buf = raw[base:base + n * 9408].view(n, 56, 56, 3)
    assert buf.data_ptr() % 128 == offset
    assert a.lib.bbai_set_render_target(a.handle, ctypes.c_void_p(buf.data_ptr())) == 0
    acts = actions_torch(9, 0, 40, 0, n, gpu)
    stream = a._stream()
    for t in range(40):
        a.step(acts[t])                       # renders into a.pixels: no longer the target, full renders
        b.step(acts[t])
        assert a.lib.bbai_render(a.handle, ctypes.c_void_p(a.image.data_ptr()), ctypes.c_void_p(buf.data_ptr()), stream) == 0
        assert torch.equal(a.pixels, b.pixels) and torch.equal(buf, b.pixels), t
    assert a.get_option("render_delta_valid") == (1 if offset == 0 else 0)
    assert raw[:base].eq(0).all() and raw[base + n * 9408:].eq(0).all()


@pytest.mark.gpu
def test_step_then_render_fallback_equals_the_fused_step(gpu, monkeypatch):
    """A library without bbai_step_render and bbai_set_render_target (an older experiment build): the binding registers no target and steps,
    then renders -- the same pixels, encodings, rewards and dones as the fused call, step for step, per-env resets included."""
    import torch
    from babyai_amd import engine
    from babyai_amd.engine import BatchedBabyAIEnv
    lacks = ("bbai_step_render", "bbai_set_render_target")

    class Older(object):
        def __init__(self, lib):
            self._real = lib

        def __getattr__(self, name):
            if name in lacks:
                raise AttributeError(name)
            return getattr(self._real, name)

    n, T, level = 65, 48, "BabyAI-GoToLocal-v0"          # a full wave plus one env
    real = engine.load_library()
    a = BatchedBabyAIEnv(level, n, device=gpu, pixel=True, seeds=31)
    _open.append(a)
    monkeypatch.setattr(engine, "_lib", Older(real))
    b = BatchedBabyAIEnv(level, n, device=gpu, pixel=True, seeds=31)
    _open.append(b)
    monkeypatch.undo()
    assert a.lib is real and all(hasattr(a.lib, name) for name in lacks)
    assert not any(hasattr(b.lib, name) for name in lacks) and hasattr(b.lib, "bbai_step")
    a.reset()
    b.reset()
    assert torch.equal(a.pixels, b.pixels) and torch.equal(a.image, b.image)
    rng = np.random.RandomState(7)
    for t in range(T):
        act = rng.randint(0, 7, size=n).astype(np.uint8)
        if t % 8 == 7:
            act[rng.choice(n, size=5, replace=False)] = BatchedBabyAIEnv.RESET_ENV
        act = torch.as_tensor(act, device=gpu)
        oa, ra, da, _ = a.step(act)
        ob, rb, db, _ = b.step(act)
        assert oa["image"] is a.pixels and ob["image"] is b.pixels
        for k in ("pixels", "image", "reward", "done"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (k, t)
