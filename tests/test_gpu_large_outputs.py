"""Every frame-writing entry with an output that crosses the 2 GiB and 4 GiB byte offsets: k_view_pixels, k_view_pixels_n, k_render_grid at
16 / 32, k_view_obs, the registered targets' delta renders (k_view_delta / k_view_ids, k_grid_delta / k_grid_ids) and the two planners'
overlap tests.  A 32-bit product in a kernel, in a launch record, in a planner or in the binding shows only beyond those offsets, as
wrong or missing bytes inside the allocation; the small-output tests cannot see it.

The counts are large_outputs_util.count_for's: the smallest with the output 16 MiB past 4 GiB, plus 3 -- a partial last launch group, a
frame across 2^31 and one across 2^32.  Every byte is compared, on the device, in slices of at most 256 MiB.
  a. listed ids with repeats: 96 distinct frames of a small batch, held to the references the suite has (view_pixels_util.frames, the
     oracle's render / gen_obs), drawn k times over in one call into a poisoned buffer between guard bands;
  b. the registered partial-view target (env.pixels at 16 / 32) against view_pixels_util.frames(env.image) after reset() and steps;
  c. the registered full-grid target (env.full at 32 / 8): twin batches with the delta render on and off, scattered envs against the oracle;
  d. a foreign render into a frame of the registered buffer beyond 4 GiB drops the history (test_what_drops_the_history at that offset).
Each case prints its wall time and the highest byte offset it verified (profiles/large_outputs/)."""
import time

import numpy as np
import pytest

import grid_delta_util as gdu
import large_outputs_util as lou
import view_pixels_util as vpu
from test_gpu_parity import _oracle_envs
from test_gpu_render_grid import Lockstep, _check

ROOM, BOSS = "GoToLocal", "BossLevel"
SMALL_N, SMALL_STEPS = 96, 40
SMALL_SEED = {ROOM: 2100, BOSS: 2200}
ACTIONS = np.array([0, 1, 2, 2, 2, 2, 3, 3, 5, 5, 4, 6], dtype=np.uint8)      # biased towards forward / pickup / toggle
BOSS_W = BOSS_H = 22
_open = []


@pytest.fixture(autouse=True)
def _release():
    yield
    while _open:
        _open.pop().close()
    import gc
    gc.collect()
    import torch
    torch.cuda.empty_cache()


def make_env(gpu, level, n, **kw):
    from babyai_amd.engine import BatchedBabyAIEnv
    e = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device=gpu, **kw)
    _open.append(e)
    return e


def record(case, t0, highest):
    import torch
    torch.cuda.synchronize()
    print("large_outputs case=%s seconds=%.2f highest_offset_verified=%d (%s)" % (case, time.time() - t0, highest, lou.where_of(highest)))


def small_actions(level):
    """uint8[SMALL_STEPS, SMALL_N]: the small batches' action stream."""
    return ACTIONS[np.random.RandomState(SMALL_SEED[level]).randint(0, len(ACTIONS), size=(SMALL_STEPS, SMALL_N))]


@pytest.fixture(scope="module")
def small(gpu):
    """level -> a Lockstep of 96 envs, 40 steps in (doors open, objects carried), with its oracle twins."""
    made = {}

    def get(level):
        if level not in made:
            ls = Lockstep(level, SMALL_N, gpu, seed=SMALL_SEED[level])
            for a in small_actions(level):
                ls.step(a)
            img = ls.env.image
            assert int(((img[:, 3, 6, 0] >= 5) & (img[:, 3, 6, 0] <= 7)).sum()) > 0, "no env of the small batch carries an object"
            if level == BOSS:
                assert any(c is not None and c.type == "door" and c.is_open for r in ls.refs for c in r.grid.grid), "no open door"
            made[level] = ls
        return made[level]
    yield get
    for ls in made.values():
        ls.env.close()


def listed_ids(k, m, F, gpu, seed, outside=True):
    """int64[k] on the device: pseudo-random ids in [0, m) -- repeats throughout --, and an id outside the batch before, at and after the
    frame across 2^31 and the one across 2^32, at both ends and in the last three rows."""
    import torch
    gen = torch.Generator(device=gpu)
    gen.manual_seed(seed)
    ids = torch.randint(0, m, (k,), dtype=torch.int64, device=gpu, generator=gen)
    if outside:
        spots = [0, k - 2]
        if k * F > lou.LIMIT_4G:
            for j in lou.straddlers(F):
                assert 1 <= j and j + 1 < k - 3
                spots += [j - 1, j, j + 1]
        bad = [-1, m, (1 << 40) + 5, -(1 << 33), m + 7]
        for i, s in enumerate(spots):
            ids[s] = bad[i % len(bad)]
    return ids


def large_call(gpu, case, shape, k, distinct, call, seed, outside=True):
    """One call that draws `k` frames listed by id into a banded, poisoned buffer; every row against `distinct`."""
    import torch
    t0 = time.time()
    F = int(np.prod(shape))
    assert tuple(distinct.shape) == (SMALL_N,) + tuple(shape) and distinct.dtype == torch.uint8
    lou.need_memory(k * F + 4 * lou.SLICE_BYTES, gpu)
    ids = listed_ids(k, SMALL_N, F, gpu, seed, outside)
    out, bands = lou.banded_out(k, shape, device=gpu)
    got = call(ids, out)
    assert got.data_ptr() == out.data_ptr()
    highest = lou.assert_rows_equal(out, distinct, ids, case)
    bands()
    if outside:
        assert not out[0].any() and not out[k - 2].any() and out[k - 1].any() and out[1].any()
    record(case, t0, highest)


# ---- a. listed ids with repeats on a small batch ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("level,ts", [(ROOM, 16), (BOSS, 32)])
def test_render_view_listed(gpu, small, level, ts):
    import torch
    env = small(level).env
    distinct = env.render_view(None, tile_size=ts)
    assert torch.equal(distinct, vpu.frames(env.image, ts))
    F = vpu.frame_bytes(7, ts)
    k = lou.count_for(F)
    assert k % 32 != 0
    large_call(gpu, "render_view[ts=%d]" % ts, (7 * ts, 7 * ts, 3), k, distinct, lambda ids, out: env.render_view(ids, tile_size=ts, out=out), ts)


@pytest.mark.gpu
@pytest.mark.parametrize("level,V,ts", [(ROOM, 11, 32), (BOSS, 3, 8)])
def test_render_view_at_a_view_size_listed(gpu, small, level, V, ts):
    """V = 11 at 32: frames of 371 712 bytes, drawn in slices.  V = 3 at 8: frames of 1 728 bytes, 2.5 million of them -- the most items a
    launch table sees."""
    import torch
    from babyai_amd import engine
    env = small(level).env
    distinct = env.render_view(None, tile_size=ts, view_size=V)
    assert torch.equal(distinct, vpu.frames(env.observe_view(None, V), ts))
    F = vpu.frame_bytes(V, ts)
    k = lou.count_for(F)
    epi, slices, items, _ = engine.view_pixels_items(V, ts, k, torch.cuda.get_device_properties(gpu).multi_processor_count)
    assert (slices > 1 and items == k * slices) if V == 11 else (epi > 1 and k % epi != 0 and k > 1 << 21), (epi, slices, items)
    large_call(gpu, "render_view[view_size=%d,ts=%d]" % (V, ts), (V * ts, V * ts, 3), k, distinct,
               lambda ids, out: env.render_view(ids, tile_size=ts, out=out, view_size=V), 100 + V)


@pytest.mark.gpu
@pytest.mark.parametrize("ts,highlight", [(32, True), (32, False), (16, True)])
def test_render_grid_listed(gpu, small, ts, highlight):
    import torch
    ls = small(BOSS)
    distinct = torch.as_tensor(_check(ls.env, ls.refs, ts, highlight, None, "the small batch"), device=gpu)
    F = gdu.frame_bytes(BOSS_W, BOSS_H, ts)
    k = lou.count_for(F)
    large_call(gpu, "render_grid[ts=%d,highlight=%d]" % (ts, highlight), (BOSS_H * ts, BOSS_W * ts, 3), k, distinct,
               lambda ids, out: ls.env.render_grid(ids, tile_size=ts, highlight=highlight, out=out), 200 + ts + highlight)


@pytest.mark.gpu
def test_render_encoding_of_a_stored_batch(gpu, small):
    """render_encoding takes rows, not ids: the stored batch is the small batch's encodings gathered k times over."""
    import torch
    ts = 32
    env = small(ROOM).env
    distinct = env.render_view(None, tile_size=ts)
    assert torch.equal(distinct, vpu.frames(env.image, ts))
    F = vpu.frame_bytes(7, ts)
    k = lou.count_for(F)
    enc = env.image.clone()

    def call(ids, out):
        stored = enc[ids].contiguous()
        assert tuple(stored.shape) == (k, 7, 7, 3)
        return env.render_encoding(stored, out=out, tile_size=ts)
    large_call(gpu, "render_encoding[ts=32]", (7 * ts, 7 * ts, 3), k, distinct, call, 300, outside=False)


@pytest.mark.gpu
def test_observe_view_listed(gpu, small):
    """2^22 + 3 frames of 363 bytes, 1.5 GB: this case is about the item count, not the byte offset."""
    import torch
    V = 11
    ls = small(BOSS)
    distinct = ls.env.observe_view(None, V)
    got = distinct.cpu().numpy()
    for i, r in enumerate(ls.refs):
        r.agent_view_size = V                        # (what ViewSizeWrapper(env, V) sets; gen_obs reads it per call)
        want = r.gen_obs()["image"]
        r.agent_view_size = 7
        assert np.array_equal(got[i], want), i
    large_call(gpu, "observe_view[view_size=11]", (V, V, 3), (1 << 22) + 3, distinct, lambda ids, out: ls.env.observe_view(ids, V, out=out), 400)


# ---- b. the registered partial-view target ------------------------------------------------------------------------------------------------
def view_batch(gpu, ts, seed=7000):
    F = vpu.frame_bytes(7, ts)
    n = lou.count_for(F)
    lou.need_memory(n * F + 6 * lou.SLICE_BYTES, gpu)
    env = make_env(gpu, ROOM, n, seeds=seed, pixel=True, tile_size=ts)
    assert tuple(env.pixels.shape) == (n, 7 * ts, 7 * ts, 3) and env.pixels.numel() > lou.LIMIT_4G + (1 << 24)
    assert env.get_option("render_target_tile_size") == ts and env.get_option("render_delta") == 1
    return env, n, F


def pixels_are_the_frames(env, ts, what):
    return lou.assert_frames_equal(env.pixels, lambda lo, hi: vpu.frames(env.image[lo:hi], ts), what)


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [1, 0])
@pytest.mark.parametrize("ts", [32, 16])
def test_registered_view_target(gpu, ts, delta):
    import torch
    t0 = time.time()
    env, n, F = view_batch(gpu, ts)
    if not delta:
        env.set_option("render_delta", 0)
    past = lou.first_frame_past(F)
    assert 0 < past < n - 3
    assert n % 16 == (8 if ts == 32 else 4)          # k_view_delta's groups of 8 / 16 envs: whole groups at 32, a partial last one at 16
    acts = torch.as_tensor(np.random.RandomState(ts + delta).randint(0, 7, size=(12, n)).astype(np.uint8), device=gpu)
    env.reset()
    highest = pixels_are_the_frames(env, ts, "reset")
    assert env.get_option("render_delta_valid") == delta
    prev = env.image.clone()
    for t in range(1, 13):
        env.step(acts[t - 1])
        if t in (1, 2, 12):
            # envs whose frames lie wholly beyond 4 GiB changed since the last comparison: the render stored there
            assert int((env.image[past:] != prev[past:]).reshape(n - past, -1).any(dim=1).sum()) > 0, t
            assert int((env.image[:past] != prev[:past]).reshape(past, -1).any(dim=1).sum()) > 0, t
            highest = pixels_are_the_frames(env, ts, "step %d" % t)
            assert env.get_option("render_delta_valid") == delta
            prev.copy_(env.image)
    record("registered_view_target[ts=%d,render_delta=%d]" % (ts, delta), t0, highest)


# ---- c. the registered full-grid target ---------------------------------------------------------------------------------------------------
def grid_batch(gpu, ts, seed, copies=1):
    F = gdu.frame_bytes(BOSS_W, BOSS_H, ts)
    n = lou.count_for(F)
    lou.need_memory(copies * n * F + 6 * lou.SLICE_BYTES, gpu)
    envs = [make_env(gpu, BOSS, n, seeds=seed, pixel=True, full_obs=True, tile_size=ts) for _ in range(copies)]
    for e in envs:
        assert e._grid_target and tuple(e.full.shape) == (n, BOSS_H * ts, BOSS_W * ts, 3) and e.full.numel() > lou.LIMIT_4G + (1 << 24)
        assert e.get_option("grid_render_delta") == 1 and e.get_option("grid_delta_valid") == 0
    return envs, n, F


def full_is_the_frames(env, ts, what):
    """env.full against whole frames of the current state, drawn a slice of envs at a time into a buffer of their own."""
    import torch

    def whole(lo, hi):
        return env.render_grid(torch.arange(lo, hi, dtype=torch.int64, device=env.device), tile_size=ts, highlight=False)
    return lou.assert_frames_equal(env.full, whole, what)


@pytest.mark.gpu
@pytest.mark.parametrize("ts", [32, 8])
def test_registered_grid_target_twins(gpu, ts):
    import torch
    t0 = time.time()
    seed = 8000 + ts
    (a, b), n, F = grid_batch(gpu, ts, seed, copies=2)
    b.set_option("grid_render_delta", 0)
    j31, j32 = lou.straddlers(F)
    assert j32 < n - 1 and n % 8 != 0
    rng = np.random.RandomState(ts)
    ends = [0, j31, j32, n - 1]
    spots = sorted(ends + [i for i in rng.permutation(n).tolist() if i not in ends][:60])           # the oracle's envs
    listed = sorted(ends[1:] + [i for i in rng.permutation(n).tolist() if i not in ends][:61])      # the envs load_state and reseed move
    assert len(spots) == len(set(spots)) == 64 and len(listed) == len(set(listed)) == 64
    refs = _oracle_envs(BOSS, [seed + i for i in spots])
    for r in refs:
        r.reset()
    acts = rng.randint(0, 7, size=(12, n)).astype(np.uint8)
    dev_acts = torch.as_tensor(acts, device=gpu)

    def same(what):
        assert a.get_option("grid_delta_valid") == 1 and b.get_option("grid_delta_valid") == 1, what
        highest = lou.assert_same(a.full, b.full, what)
        assert torch.equal(a.grid_shadow(), b.grid_shadow()), what
        return highest

    def oracle(what, which=None):
        sel = [k for k, i in enumerate(spots) if which is None or i in which]
        got = a.full[torch.as_tensor([spots[k] for k in sel], device=gpu)].cpu().numpy()
        for g, k in zip(got, sel):
            want = refs[k].render("rgb_array", highlight=False, tile_size=ts)
            assert np.array_equal(g, want), (what, spots[k], lou.where_of(spots[k] * F))

    a.reset(), b.reset()
    same("reset")
    oracle("reset", {0, j31, j32, n - 1})
    snaps = None
    for t in range(12):
        a.step(dev_acts[t]), b.step(dev_acts[t])
        dn = a.done[torch.as_tensor(spots, device=gpu)].cpu().numpy()
        for k, i in enumerate(spots):
            _, _, d, _ = refs[k].step(int(acts[t, i]))
            assert bool(d) == bool(dn[k]), (t, i)
            if d:
                refs[k].reset()
        same("step %d" % t)
        if t == 5:
            snaps = a.save_state(listed), b.save_state(listed)
    oracle("12 steps")
    full_is_the_frames(a, ts, "12 steps")
    for env, snap in zip((a, b), snaps):
        env.load_state(snap, listed)
    same("load_state")
    full_is_the_frames(a, ts, "load_state")
    seeds = [90000 + i for i in range(len(listed))]
    for env in (a, b):
        env.reseed(listed, seeds)
    highest = same("reseed")
    full_is_the_frames(a, ts, "reseed")
    fresh = _oracle_envs(BOSS, [seeds[listed.index(i)] for i in (j31, j32, n - 1)])
    got = a.full[torch.as_tensor([j31, j32, n - 1], device=gpu)].cpu().numpy()
    for g, r, i in zip(got, fresh, (j31, j32, n - 1)):
        r.reset()
        assert np.array_equal(g, r.render("rgb_array", highlight=False, tile_size=ts)), ("reseed", i)
    a.step(dev_acts[0]), b.step(dev_acts[0])
    same("a step behind the reseed")
    record("registered_grid_target_twins[ts=%d]" % ts, t0, highest)


# ---- d. history drops at high addresses ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_render_into_a_frame_of_pixels_beyond_4_gib_drops_the_history(gpu):
    import torch
    t0 = time.time()
    ts = 32
    env, n, F = view_batch(gpu, ts, seed=7100)
    slot = n - 2
    assert slot * F >= lou.LIMIT_4G and slot >= lou.first_frame_past(F)
    acts = torch.as_tensor(np.random.RandomState(5).randint(0, 7, size=(2, n)).astype(np.uint8), device=gpu)
    env.reset()
    env.step(acts[0])
    assert env.get_option("render_delta_valid") == 1
    assert not torch.equal(env.image[0], env.image[slot])
    env.render_view([0], tile_size=ts, out=env.pixels[slot:slot + 1])          # env 0's frame where env n - 2's stood
    assert env.get_option("render_delta_valid") == 0, "a write into the registered buffer beyond 4 GiB left its history valid"
    env.step(acts[1])
    assert env.get_option("render_delta_valid") == 1
    highest = pixels_are_the_frames(env, ts, "the step behind the foreign render")
    env.render_view([0], tile_size=ts)                                         # ... and one into a buffer of its own keeps it
    assert env.get_option("render_delta_valid") == 1
    record("history_drop[pixels,ts=32]", t0, highest)


@pytest.mark.gpu
def test_a_render_into_a_frame_of_full_beyond_4_gib_drops_the_history(gpu):
    import torch
    t0 = time.time()
    ts = 32
    (env,), n, F = grid_batch(gpu, ts, 8100)
    slot = n - 2
    assert slot * F >= lou.LIMIT_4G
    acts = torch.as_tensor(np.random.RandomState(6).randint(0, 7, size=(2, n)).astype(np.uint8), device=gpu)
    env.reset()
    env.step(acts[0])
    assert env.get_option("grid_delta_valid") == 1
    env.render_grid([0], tile_size=ts, highlight=False, out=env.full[slot:slot + 1])
    assert env.get_option("grid_delta_valid") == 0, "a write into the registered buffer beyond 4 GiB left its history valid"
    env.step(acts[1])
    assert env.get_option("grid_delta_valid") == 1
    highest = full_is_the_frames(env, ts, "the step behind the foreign render")
    env.render_grid([0], tile_size=ts, highlight=False)
    assert env.get_option("grid_delta_valid") == 1
    record("history_drop[full,ts=32]", t0, highest)
