"""Partial-view pixels at view sizes 3, 5, 7, 9, 11 and tile sizes 8, 16, 32 on the device (k_view_pixels_n<V, TS>,
include/bbai_view_pixels.h bbai_render_view_pixels; render_encoding / render_view with view_size=V): byte for byte against a gather
written from the picture's geometry and the atlas files alone (view_pixels_util, which tests/test_view_pixels_host.py holds to the
oracle's get_obs_render), against the 7x7 entries at V = 7, and from the state against the oracle itself; the launch's edge shapes, id
lists, the registered render target and every refusal."""
import ctypes

import numpy as np
import pytest

import view_pixels_util as vpu

COMBOS = [(V, ts) for V in vpu.VIEW_SIZES for ts in vpu.TILE_SIZES]
OTHER = (3, 5, 9, 11)
LEVELS = ("GoToLocal", "BossLevel", "OpenRedDoor", "PutNextS5N2Carrying")
ACTIONS = np.array([0, 1, 2, 2, 2, 2, 3, 3, 5, 5, 4, 6], dtype=np.uint8)      # biased towards forward / pickup / toggle
GUARD = 4096


@pytest.fixture(scope="module")
def env(gpu):
    """One small encoded batch whose handle every synthetic case draws with."""
    from babyai_amd.engine import BatchedBabyAIEnv
    e = BatchedBabyAIEnv("BabyAI-GoToLocal-v0", 8, device=gpu, seeds=1)
    e.reset()
    yield e
    e.close()


def _guarded(env, V, ts, k):
    """uint8[k, V ts, V ts, 3] inside a buffer with GUARD bytes of 0xAB on both sides (the frames start 16-byte aligned)."""
    import torch
    nbytes = k * vpu.frame_bytes(V, ts)
    buf = torch.full((nbytes + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=env.device)
    return buf, buf[GUARD:GUARD + nbytes].view(k, V * ts, V * ts, 3)


def _guards_untouched(buf):
    return bool((buf[:GUARD] == 0xAB).all()) and bool((buf[-GUARD:] == 0xAB).all())


def _counts(V, ts, cus):
    """1; one more than a full-size item holds (a count this small is spread over single-frame items, or slices: the launch keeps an item
    per block); more full-size items than persistent blocks plus a remainder (a block goes through a second item and the other id plane,
    and the last item is a partial one) -- from the launch's own item table."""
    from babyai_amd import engine
    epi, slices, _, _ = engine.view_pixels_items(V, ts, 1 << 40, cus)      # the full-size shape: count no longer limits an item
    blocks = cus * engine.VIEW_PIXELS_BLOCKS_PER_CU
    large = (blocks + 3) * epi + 1 if slices == 1 else blocks // slices + 2
    for count in (epi + 1, large):
        e, s, items, nb = engine.view_pixels_items(V, ts, count, cus)
        if count == large:
            assert (e, s) == (epi, slices) and items > nb == blocks and (epi == 1 or count % epi == 1), (V, ts, count)
    return 1, epi + 1, large


@pytest.mark.gpu
@pytest.mark.parametrize("V,ts", COMBOS)
def test_every_tile_at_every_size(gpu, env, V, ts):
    import torch
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    counts = _counts(V, ts, cus)
    assert counts[2] >= 19                                                   # every carried object on the agent's cell
    enc = torch.as_tensor(vpu.synthetic_encodings(counts[2], V, 7 * V + ts), device=gpu)
    want = vpu.frames(enc, ts)                                               # (built on the device, once for the three counts)
    assert len(torch.unique(vpu.tile_ids(enc, ts))) == 58                    # every tile of the atlas: 39 ordinary cells + 19 carried objects
    for k in counts:
        buf, out = _guarded(env, V, ts, k)
        got = env.render_encoding(enc[:k], out=out, tile_size=ts, view_size=V) if V != 7 else env._view_pixels_into(enc[:k], None, k, V, ts, out)
        assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (k, V * ts, V * ts, 3)
        bad = torch.nonzero((got != want[:k]).reshape(k, -1).any(dim=1)).reshape(-1)
        assert len(bad) == 0, (V, ts, k, bad[:8].tolist())
        assert _guards_untouched(buf), (V, ts, k)
    alloc = env.render_encoding(enc[:3], tile_size=ts, view_size=V) if V != 7 else None      # `out` allocated when none is given
    assert alloc is None or torch.equal(alloc, want[:3])


@pytest.mark.gpu
@pytest.mark.parametrize("V,ts", [(3, 8), (5, 8), (9, 8), (5, 16), (11, 32)])
def test_id_lists(gpu, env, V, ts):
    import torch
    rows = 45
    enc = torch.as_tensor(vpu.synthetic_encodings(rows, V, 3), device=gpu)
    want = vpu.frames(enc, ts)
    lists = [list(range(rows - 1, -1, -1)), [5, 5, 44, 3, 5, 0, 5], [7, -1, rows, 1 << 40, 2, -(1 << 40), rows + 7, 7] + list(range(30, 9, -1)), []]
    side = torch.cuda.Stream(device=gpu)
    for ids in lists:
        for stream in (None, side):
            k = len(ids)
            buf, out = _guarded(env, V, ts, k)
            ids_t = torch.as_tensor(np.asarray(ids, dtype=np.int64), device=gpu)
            torch.cuda.synchronize()
            s = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
            rc = env.lib.bbai_render_view_pixels(env.handle, V, ts, enc.data_ptr(), rows, ids_t.data_ptr() if k else None, k,
                                                 out.data_ptr() if k else None, s)
            assert rc == 0, (ids, env.lib.bbai_last_error())
            torch.cuda.synchronize()
            for j, i in enumerate(ids):
                assert torch.equal(out[j], want[i] if 0 <= i < rows else torch.zeros_like(out[j])), (V, ts, j, i)
            assert _guards_untouched(buf)
    # the encodings were only read
    assert torch.equal(enc, torch.as_tensor(vpu.synthetic_encodings(rows, V, 3), device=gpu))


@pytest.mark.gpu
@pytest.mark.parametrize("ts", vpu.TILE_SIZES)
def test_view_size_7_is_the_7x7_entries_picture(gpu, ts):
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    n = 77
    e = BatchedBabyAIEnv("BabyAI-BossLevel-v0", n, device=gpu, seeds=11)
    e.reset()
    a = torch.as_tensor(ACTIONS[np.random.RandomState(2).randint(0, len(ACTIONS), size=(5, n))], device=gpu)
    for t in range(5):
        e.step(a[t])
    e._install_atlas("view", ts)                   # (render_encoding at 8 on an encoded batch expects bbai_render's atlas in place)
    for enc in (e.image, torch.as_tensor(vpu.synthetic_encodings(n, 7, 5), device=gpu)):
        old = e.render_encoding(enc, out=torch.empty((n, 7 * ts, 7 * ts, 3), dtype=torch.uint8, device=gpu), tile_size=ts).clone()
        new = e._view_pixels_into(enc, None, n, 7, ts, torch.empty((n, 7 * ts, 7 * ts, 3), dtype=torch.uint8, device=gpu))
        assert torch.equal(new, old)
    # render_view(view_size=7) given explicitly: the listed envs natively, the default call's bytes
    ids = [3, 3, 76, -1, 0, n, 41]
    assert torch.equal(e.render_view(ids, tile_size=ts, view_size=7), e.render_view(ids, tile_size=ts))
    assert torch.equal(e.render_view(tile_size=ts, view_size=7), e.render_view(tile_size=ts))
    e.close()


def _oracle_views(level, seeds, V):
    """Oracle envs with agent_view_size = V set before seed() / reset(): what ViewSizeWrapper(env, V) does."""
    from oracle import levels as olevels
    refs = []
    for s in seeds:
        r = olevels.make_env(level)
        r.agent_view_size = V
        r.seed(int(s))
        refs.append(r)
    return refs


@pytest.mark.gpu
@pytest.mark.parametrize("V", OTHER)
@pytest.mark.parametrize("level", LEVELS)
def test_render_view_from_the_state_matches_the_oracle(gpu, level, V):
    """render_view(ids, tile_size, view_size=V) on an encoded batch and on a view_size=V batch (ids=None: the self.view path) against
    get_obs_render of oracle envs with agent_view_size = V, at reset() and along random steps with auto-reset; the view_size batch's
    step() outputs equal a twin's that never renders."""
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    n, steps, seed = 16, 30, 500 + V
    seeds = [seed + i for i in range(n)]
    enc_env = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device=gpu, seeds=seed)
    view_env = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device=gpu, seeds=seed, view_size=V)
    twin = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device=gpu, seeds=seed, view_size=V)
    refs = _oracle_views(level, seeds, V)
    obs_ref = [r.reset() for r in refs]
    enc_env.reset()
    view_env.reset()
    twin.reset()
    rng = np.random.RandomState(V)
    order = list(range(n - 1, -1, -1))
    for t in range(steps + 1):
        ts = vpu.TILE_SIZES[t % 3] if t else 8
        for tile in (vpu.TILE_SIZES if t == 0 else (ts,)):
            want = np.stack([refs[i].get_obs_render(obs_ref[i]["image"], tile_size=tile) for i in range(n)])
            got_enc = enc_env.render_view(order, tile_size=tile, view_size=V).cpu().numpy()
            got_view = view_env.render_view(tile_size=tile, view_size=V).cpu().numpy()
            assert got_view.shape == want.shape == (n, V * tile, V * tile, 3)
            assert np.array_equal(got_enc, want[::-1]), (level, V, tile, t)
            assert np.array_equal(got_view, want), (level, V, tile, t)
        if t == steps:
            break
        a = ACTIONS[rng.randint(0, len(ACTIONS), size=n)]
        at = torch.as_tensor(a, device=gpu)
        enc_env.step(at)
        o1, r1, d1, _ = view_env.step(at)
        o2, r2, d2, _ = twin.step(at)
        assert torch.equal(o1["image"], o2["image"]) and torch.equal(r1, r2) and torch.equal(d1, d2) and torch.equal(view_env.direction, twin.direction)
        assert torch.equal(view_env.image, twin.image)
        dn = d1.cpu().numpy()
        for i in range(n):
            o, _, d, _ = refs[i].step(int(a[i]))
            assert bool(d) == bool(dn[i]), (t, i)
            obs_ref[i] = refs[i].reset() if d else o
    # ids outside the batch: zero frames; another view size than the batch's own, and a listed render on the view_size batch
    got = view_env.render_view([2, -1, n, 2], tile_size=16, view_size=V)
    assert torch.equal(got[0], got[3]) and not got[1].any() and not got[2].any() and got[0].any()
    other = 5 if V != 5 else 9
    assert torch.equal(view_env.render_view(tile_size=8, view_size=other), enc_env.render_view(tile_size=8, view_size=other))
    # view_size=None is the 7x7 view of self.image on every batch
    assert torch.equal(view_env.render_view(tile_size=16), enc_env.render_view(tile_size=16))
    assert tuple(view_env.render_view([], tile_size=8, view_size=V).shape) == (0, V * 8, V * 8, 3)
    for e in (enc_env, view_env, twin):
        e.close()


@pytest.mark.gpu
def test_a_render_into_the_registered_target_invalidates_its_history(gpu):
    """pixel=True, tile_size=16: env.pixels is the registered target.  A new-entry render whose output lies inside it is a foreign write --
    the next step() redraws every frame whole, so env.pixels is again the picture of env.image; a render elsewhere leaves the history
    alone and the step's delta render still arrives at the same picture."""
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    n, ts = 64, 16
    for inside in (True, False):
        e = BatchedBabyAIEnv("BabyAI-GoToLocal-v0", n, device=gpu, seeds=9, pixel=True, tile_size=ts)
        e.reset()
        a = torch.as_tensor(ACTIONS[np.random.RandomState(4).randint(0, len(ACTIONS), size=(4, n))], device=gpu)
        e.step(a[0])
        e.step(a[1])                                   # (the target's history is valid by now)
        enc = torch.as_tensor(vpu.synthetic_encodings(10, 5, 1), device=gpu)
        k = 10
        nbytes = k * vpu.frame_bytes(5, ts)
        if inside:
            off = 3 * vpu.frame_bytes(7, ts) + 64      # in the middle of env 3's frame
            out = e.pixels.view(-1)[off:off + nbytes].view(k, 5 * ts, 5 * ts, 3)
        else:
            out = torch.empty((k, 5 * ts, 5 * ts, 3), dtype=torch.uint8, device=gpu)
        got = e.render_encoding(enc, out=out, tile_size=ts, view_size=5)
        assert torch.equal(got, vpu.frames(enc, ts))
        # make every env's picture change, so that stale bytes could only survive under a delta render that trusts the history
        e.step(a[2])
        e.step(a[3])
        want = vpu.frames(e.image, ts)
        assert torch.equal(e.pixels, want), inside
        e.close()


@pytest.mark.gpu
def test_refusals(gpu):
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv, EngineError
    e = BatchedBabyAIEnv("BabyAI-GoToLocal-v0", 4, device=gpu, seeds=1)
    e.reset()
    lib, h = e.lib, e.handle
    V, ts, rows = 5, 16, 4
    fb = vpu.frame_bytes(V, ts)
    enc = torch.as_tensor(vpu.synthetic_encodings(rows, V, 2), device=gpu)
    out = torch.full((rows * fb + 32,), 0xAB, dtype=torch.uint8, device=gpu)
    img, o = enc.data_ptr(), out.data_ptr()
    ARG, STATE = -1, -3
    assert lib.bbai_render_view_pixels(h, V, ts, img, rows, None, rows, o, None) == STATE      # no atlas of that size yet
    tiles, lut = vpu.atlas(ts)
    assert lib.bbai_set_view_pixels_atlas(h, 12, tiles.ctypes.data, 58, lut.ctypes.data) == ARG
    assert lib.bbai_set_view_pixels_atlas(h, 64, tiles.ctypes.data, 58, lut.ctypes.data) == ARG
    assert lib.bbai_set_view_pixels_atlas(h, ts, tiles.ctypes.data, 0, lut.ctypes.data) == ARG
    assert lib.bbai_set_view_pixels_atlas(h, ts, tiles.ctypes.data, 65, lut.ctypes.data) == ARG
    assert lib.bbai_set_view_pixels_atlas(h, ts, tiles.ctypes.data, 57, lut.ctypes.data) == ARG   # a lut entry names tile 57
    assert lib.bbai_set_view_pixels_atlas(h, ts, None, 58, lut.ctypes.data) == ARG
    assert lib.bbai_set_view_pixels_atlas(h, ts, tiles.ctypes.data, 58, None) == ARG
    assert lib.bbai_render_view_pixels(h, V, ts, img, rows, None, rows, o, None) == STATE         # (a refused install installs nothing)
    assert lib.bbai_set_view_pixels_atlas(h, ts, tiles.ctypes.data, 58, lut.ctypes.data) == 0
    assert lib.bbai_render_view_pixels(h, V, 8, img, rows, None, rows, o, None) == STATE          # (each size has its own)
    assert lib.bbai_render_view_pixels(h, V, 32, img, rows, None, rows, o, None) == STATE
    for bad_v in (4, 13, 0, -5):
        assert lib.bbai_render_view_pixels(h, bad_v, ts, img, rows, None, rows, o, None) == ARG
    for bad_ts in (12, 64, 0):
        assert lib.bbai_render_view_pixels(h, V, bad_ts, img, rows, None, rows, o, None) == ARG
    assert lib.bbai_render_view_pixels(h, V, ts, img, rows, None, rows, o + 8, None) == ARG       # misaligned
    assert lib.bbai_render_view_pixels(h, V, ts, img, rows, None, rows, None, None) == ARG
    assert lib.bbai_render_view_pixels(h, V, ts, img, rows, None, rows + 1, o, None) == ARG       # count > rows without ids
    assert lib.bbai_render_view_pixels(h, V, ts, img, rows, None, -1, o, None) == ARG
    assert lib.bbai_render_view_pixels(h, V, ts, img, -1, None, 0, o, None) == ARG
    assert lib.bbai_render_view_pixels(h, V, ts, None, rows, None, rows, o, None) == ARG          # no encodings, work to do
    assert lib.bbai_render_view_pixels(h, V, ts, img, rows, None, 0, None, None) == 0
    assert lib.bbai_render_view_pixels(h, V, ts, None, 0, None, 0, None, None) == 0
    torch.cuda.synchronize()
    assert bool((out == 0xAB).all())                                                              # a refused call writes nothing
    # the 7x7 entries' atlases are not this entry's (and the other way round)
    assert lib.bbai_render_view(h, ts, e.image.data_ptr(), 4, None, 4, o, None) == STATE
    assert lib.bbai_render_view_pixels(h, V, ts, img, rows, None, rows, o, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:rows * fb].view(rows, V * ts, V * ts, 3), vpu.frames(enc, ts))
    assert bool((out[rows * fb:] == 0xAB).all())
    # Python: bad values raise ValueError before any launch; the installed atlases are as they were
    before = set(e._atlases)
    for kw in (dict(view_size=4), dict(view_size=13), dict(view_size="9"), dict(view_size=True), dict(view_size=9, tile_size=12),
               dict(view_size=9, tile_size=64)):
        with pytest.raises(ValueError):
            e.render_view(**kw)
        with pytest.raises(ValueError):
            e.render_encoding(enc, **kw)
    with pytest.raises(ValueError):
        e.render_encoding(enc, view_size=9, tile_size=8)                                           # uint8[k, 5, 5, 3] is no 9x9 encoding
    with pytest.raises(ValueError):
        e.render_encoding(None, view_size=9, tile_size=8)
    with pytest.raises(ValueError):
        e.render_view(view_size=9, tile_size=8, out=torch.empty((4, 56, 56, 3), dtype=torch.uint8, device=gpu))
    assert set(e._atlases) == before

    class Old(object):                                 # a library without the entries
        def __getattr__(self, name):
            if name in ("bbai_set_view_pixels_atlas", "bbai_render_view_pixels"):
                raise AttributeError(name)
            return getattr(lib, name)
    e.lib = Old()
    with pytest.raises(EngineError, match="bbai_render_view_pixels"):
        e.render_view(view_size=9, tile_size=32)
    e.lib = lib
    e.close()
