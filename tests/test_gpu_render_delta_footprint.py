"""The delta render's exact store footprint under chosen dirty cells (k_render_delta, k_render_dstore and step_dirty at
the tail of k_step), through the public ABI alone.  The other render tests compare a delta path with a full render of the same frame over a
buffer that already holds the previous frame: a kernel that stores too much writes identical bytes, one that stores too little is hidden
wherever the skipped bytes did not change.  Here the test owns the registered buffer and, before every delta render, overwrites the frame
region with Q = 255 - (the new frame), which differs from the new frame in every byte: afterwards the region must hold the new frame exactly
in the bytes the render has to store (tests/render_util.py stored_mask: the 64-byte pieces / 128-byte lines that show a changed cell) and Q
everywhere else, and the 256-byte bands in front of and behind the region must be untouched.  The dirty cells are chosen, not met: env i
gets pattern (i + shift) % 57 of render_util's catalogue (nothing, each single cell, all cells, only the cells of the 128-byte line an even
env shares with the next one, only those of the odd env, seeded subsets, whole clean 32-env groups), so every pattern meets every position
of a group, of an 8-env unit and of a pair.  The reference side is pinned without a GPU in tests/test_render_footprint_host.py, which also
checks every case's preconditions; each case asserts them again from its own inputs."""
import ctypes

import numpy as np
import pytest

import render_util as ru
from render_util import PIX_BYTES

BOSS = "BabyAI-BossLevel-v0"        # the classic layout
ROOM = "BabyAI-GoToLocal-v0"        # a single room: the in-place layout
BAND, BAND_BYTE = 256, 0xA5
SMALL = [1, 7, 8, 9, 31, 32, 33, 65]
CONFIGS = [(512, 0), (512, 1), (1024, 0)]        # (render_delta_tpb, render_delta_sched)
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


def make_env(gpu, level, n, **kw):
    from babyai_amd.engine import BatchedBabyAIEnv
    e = BatchedBabyAIEnv(level, n, device=gpu, **kw)
    _open.append(e)
    return e


def set_option(env, name, value):
    env.set_option(name, value)
    assert env.get_option(name) == value, name


class Target(object):
    """The test's own render target: one allocation of 256 + N * 9408 + 256 bytes, the frame region on a 128-byte boundary and registered
    with the handle, both bands filled with 0xA5."""

    def __init__(self, env, gpu):
        import torch
        self.n = n = env.num_envs
        self.raw = torch.full((BAND + n * PIX_BYTES + BAND,), BAND_BYTE, dtype=torch.uint8, device=gpu)
        self.frame = self.raw[BAND:BAND + n * PIX_BYTES]
        assert self.frame.data_ptr() % 128 == 0
        assert env.lib.bbai_set_render_target(env.handle, ctypes.c_void_p(self.frame.data_ptr())) == 0
        assert env.get_option("render_delta") == 1 and env.get_option("render_delta_valid") == 0

    def bands_untouched(self):
        return bool(self.raw[:BAND].eq(BAND_BYTE).all()) and bool(self.raw[BAND + self.n * PIX_BYTES:].eq(BAND_BYTE).all())


class Ref(object):
    """render_util's reference on the host (numpy) or, for the large case, on the device (torch): the same tile_ids / frames / stored_mask."""

    def __init__(self, gpu, on_device):
        self.gpu, self.on_device = gpu, on_device

    def ids(self, enc):
        import torch
        ids = ru.tile_ids(enc)                                            # (numpy, on the host)
        return torch.as_tensor(ids, device=self.gpu) if self.on_device else ids

    def flat_frames(self, ids):
        return ru.frames(ids).reshape(-1)

    def expected(self, old_ids, new_ids, unit, q):
        import torch
        mask = ru.stored_mask(old_ids, new_ids, unit)
        frac = int(mask.sum()) / float(len(mask))
        assert 0.01 <= frac <= 0.60, frac                                 # neither branch below is vacuous
        new = self.flat_frames(new_ids)
        return (torch.where(mask, new, q) if self.on_device else np.where(mask, new, q)), mask

    def put(self, target, flat):
        import torch
        target.frame.copy_(flat if self.on_device else torch.as_tensor(flat, device=self.gpu))

    def same(self, target, flat, mask=None, q=None):
        import torch
        got = target.frame if self.on_device else target.frame.cpu().numpy()
        if (torch.equal(got, flat) if self.on_device else np.array_equal(got, flat)):
            return True
        if not self.on_device and mask is not None:                       # what went wrong, for the report
            extra = np.nonzero((got != q) & ~mask)[0]
            missing = np.nonzero((got != flat) & mask)[0]
            where = lambda b: "env %d byte %d" % (b // PIX_BYTES, b % PIX_BYTES)
            print("bytes stored outside the mask: %d%s; bytes of the mask not stored (or wrong): %d%s"
                  % (len(extra), " (first: %s)" % where(extra[0]) if len(extra) else "", len(missing), " (first: %s)" % where(missing[0]) if len(missing) else ""))
        elif mask is not None:
            print("bytes stored outside the mask: %d; bytes of the mask not stored (or wrong): %d"
                  % (int(((got != q) & ~mask).sum()), int(((got != flat) & mask).sum())))
        return False

    def same_ids(self, shadow, ids):
        import torch
        return torch.equal(shadow, ids) if self.on_device else np.array_equal(shadow.cpu().numpy(), ids)


def render(env, enc, target):
    """bbai_render of a hand-made encoding (numpy uint8[N, 7, 7, 3]) into the registered target."""
    import torch
    dev = torch.as_tensor(np.ascontiguousarray(enc), device=target.raw.device)
    assert env.lib.bbai_render(env.handle, ctypes.c_void_p(dev.data_ptr()), ctypes.c_void_p(target.frame.data_ptr()), env._stream()) == 0
    torch.cuda.synchronize()                                              # (`dev` lives until the render has run)


_patterns = {}


def case_patterns(case, k):
    """Transition k's dirty cells, bool[n, 49], their preconditions asserted (once per case and transition: the tests share them)."""
    if (case.n, k) not in _patterns:
        pat, kind = case.patterns(k)
        ru.check_patterns(pat, kind, **case.conditions(k))
        _patterns[case.n, k] = pat
    return _patterns[case.n, k]


# ---- the render finds the dirty cells itself: k_render_delta -------------------------------------------------------------------------
def render_side(gpu, n, unit, configs):
    case = ru.CASE[n]
    ref = Ref(gpu, case.large)
    env = make_env(gpu, ROOM, n, pixel=True, seeds=3)
    env.reset()
    set_option(env, "render_piece_bytes", unit)
    if case.large:
        set_option(env, "render_delta_bpc", 1)                            # at most 256 blocks: five or six 32-env groups each
    target = Target(env, gpu)
    for ci, (tpb, sched) in enumerate(configs):
        set_option(env, "render_delta_tpb", tpb)
        set_option(env, "render_delta_sched", sched)
        encs = [ru.synthetic_encodings(n, 10 * n + ci)]
        for k in (0, 1):
            encs.append(ru.perturb(encs[-1], case_patterns(case, k), seed=100 * ci + k))
        ids = [ref.ids(e) for e in encs]
        render(env, encs[0], target)                                      # a full render: every byte, every tile id of the shadow
        assert env.get_option("render_delta_valid") == 1
        assert ref.same(target, ref.flat_frames(ids[0])) and ref.same_ids(env.render_shadow(), ids[0]) and target.bands_untouched()
        for k in (1, 2):                                                  # S0 -> S1, then S1 -> S2 from the shadow the first one left
            q = 255 - ref.flat_frames(ids[k])
            ref.put(target, q)
            render(env, encs[k], target)
            exp, mask = ref.expected(ids[k - 1], ids[k], unit, q)
            assert ref.same(target, exp, mask, q), (n, unit, tpb, sched, k)
            assert ref.same_ids(env.render_shadow(), ids[k]), (n, unit, tpb, sched, k)
            assert target.bands_untouched(), (n, unit, tpb, sched, k)
            assert env.get_option("render_delta_valid") == 1
        env.render_invalidate()
        assert env.get_option("render_delta_valid") == 0


@pytest.mark.gpu
@pytest.mark.parametrize("unit", [64, 128])
@pytest.mark.parametrize("n", SMALL)
def test_render_side_footprint(gpu, n, unit):
    render_side(gpu, n, unit, CONFIGS)


@pytest.mark.gpu
@pytest.mark.parametrize("tpb,sched", CONFIGS)
@pytest.mark.parametrize("unit", [64, 128])
def test_render_side_footprint_large(gpu, unit, tpb, sched):
    render_side(gpu, ru.LARGE_N, unit, [(tpb, sched)])


# ---- the step finds the dirty cells, the render only stores: step_dirty + k_render_dstore ---------------------------------------------
def step_actions(seed, steps, n, gpu):
    """Random actions; env i is told to reset (action 7) at step t where (7 i + t) % 11 == 0 -- env 0 at step 0: resets cross every run."""
    import torch
    from babyai_amd.action_stream import actions_torch
    acts = actions_torch(seed, 0, steps, 0, n, gpu)
    i = torch.arange(n, device=gpu).unsqueeze(0)
    t = torch.arange(steps, device=gpu).unsqueeze(1)
    return torch.where((7 * i + t) % 11 == 0, torch.full_like(acts, 7), acts)


def from_step(gpu, level, n, units, auto_reset=True, split=0):
    import torch
    case = ru.CASE[n]
    ref = Ref(gpu, case.large)
    a = make_env(gpu, level, n, pixel=True, seeds=41, auto_reset=auto_reset)
    b = make_env(gpu, level, n, seeds=41, auto_reset=auto_reset)          # the same envs, no pixels: the encodings the steps must give
    set_option(a, "render_delta_from_step", 1)
    set_option(a, "step_render_split", split)
    if split:
        assert n // 64 // 2 > 0 and n % 64 != 0                           # a first half of whole step blocks, the second one at an env offset
    if case.large:
        set_option(a, "render_delta_bpc", 1)
    if level == BOSS and auto_reset:
        for e in (a, b):
            set_option(e, "consume_fused", 1)                             # (the mazes' default, said out loud: k_step's rows are the final observations)
    assert a.get_option("inplace") == (1 if level == ROOM else 0)
    a.reset()
    b.reset()
    target = Target(a, gpu)
    steps = len(case.shifts)
    acts = step_actions(17, steps * len(units), n, gpu)
    finished = t = 0
    for unit in units:
        set_option(a, "render_piece_bytes", unit)
        for k in range(steps):
            b.step(acts[t])
            new_enc = b.image.cpu().numpy()                               # E'
            old_enc = ru.perturb(new_enc, case_patterns(case, k), seed=t)
            old_ids, new_ids = ref.ids(old_enc), ref.ids(new_enc)
            render(a, old_enc, target)                                    # the shadow: ids(S); the step will find exactly the perturbed cells dirty
            assert a.get_option("render_delta_valid") == 1 and ref.same_ids(a.render_shadow(), old_ids)
            q = 255 - ref.flat_frames(new_ids)
            ref.put(target, q)
            P = lambda x: ctypes.c_void_p(x.data_ptr())
            assert a.lib.bbai_step_render(a.handle, P(acts[t]), P(a.image), P(a.direction), P(a.reward), P(a.reward64), P(a.done),
                                          1 if auto_reset else 0, P(target.frame), a._stream()) == 0
            torch.cuda.synchronize()
            exp, mask = ref.expected(old_ids, new_ids, unit, q)
            assert ref.same(target, exp, mask, q), (level, n, unit, t)
            assert torch.equal(a.image, b.image) and torch.equal(a.done, b.done) and torch.equal(a.reward64, b.reward64), (level, n, unit, t)
            assert ref.same_ids(a.render_shadow(), new_ids), (level, n, unit, t)
            assert target.bands_untouched(), (level, n, unit, t)
            assert a.get_option("render_delta_valid") == 1
            finished += int(a.done.sum())
            t += 1
    assert finished > 0
    a.render_invalidate()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("level", [ROOM, BOSS])
def test_from_step_footprint(gpu, level, n):
    from_step(gpu, level, n, [64, 128])


@pytest.mark.gpu
@pytest.mark.parametrize("unit", [64, 128])
@pytest.mark.parametrize("level", [ROOM, BOSS])
def test_from_step_footprint_large(gpu, level, unit):
    from_step(gpu, level, ru.LARGE_N, [unit])


@pytest.mark.gpu
def test_from_step_footprint_frozen_envs(gpu):
    """auto_reset=False: finished envs (here: the ones told to reset) freeze and re-emit their observation."""
    from_step(gpu, BOSS, 65, [64, 128], auto_reset=False)


@pytest.mark.gpu
def test_from_step_footprint_split(gpu):
    """bbai_step_render in two halves: 64 envs, then 101 at an env offset of 64 -- masks, shadow rows and pixels of the second render start there."""
    from_step(gpu, BOSS, 128 + 37, [64, 128], split=1)
