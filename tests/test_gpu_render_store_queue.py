"""The store-only delta render with a loader wave (k_render_dstore_lw): eight waves that only store, a ninth that only
loads, a group's dirty envs handed to the storing waves as they come free, groups handed to blocks by a ticket counter.  It must store
what the static kernel stores (k_render_dstore, option "render_delta_sched" 2): every test steps a handle on the new path (0), one on the
old (2) and one that renders every frame in full ("render_delta" 0) with the same actions and compares pixels, encodings and the shadow's
tile ids after every step, byte for byte; the footprint test owns the registered buffer and checks that exactly the expected 64-byte
pieces were written (the protocol of tests/test_gpu_render_delta_footprint.py, whose helpers it uses).  Env counts: a single env, ragged
groups, odd group counts (a ticket is two groups: the last one may hold one), fewer tickets than blocks, many tickets per block."""
import ctypes

import numpy as np
import pytest

import render_util as ru
import test_gpu_render_delta_footprint as fp

BOSS = fp.BOSS
HOLD, RESET_ENV = 8, 7


@pytest.fixture(autouse=True)
def _close_handles():
    yield
    while fp._open:
        fp._open.pop().close()
    import gc
    gc.collect()
    try:
        import torch
        torch.cuda.empty_cache()
    except Exception:
        pass


def trio(gpu, n, seeds=23, bpc=0, split=0, hold=False):
    """(new path, old path, full renders): the same envs three times."""
    new = fp.make_env(gpu, BOSS, n, pixel=True, seeds=seeds)
    old = fp.make_env(gpu, BOSS, n, pixel=True, seeds=seeds)
    full = fp.make_env(gpu, BOSS, n, pixel=True, seeds=seeds)
    for e, sched in ((new, 0), (old, 2)):
        fp.set_option(e, "render_delta_from_step", 1)
        fp.set_option(e, "render_delta_sched", sched)
        fp.set_option(e, "render_delta_bpc", bpc)
        fp.set_option(e, "step_render_split", split)
        assert e.get_option("render_delta") == 1 and e.get_option("render_piece_bytes") == 64
    fp.set_option(full, "render_delta", 0)
    for e in (new, old, full):
        if hold:
            fp.set_option(e, "step_hold", 1)
        e.reset()
    return new, old, full


def same(new, old, full, where):
    import torch
    ids = ru.tile_ids(full.image)
    for name, e in (("new", new), ("old", old)):
        assert e.get_option("render_delta_valid") == 1, (name, where)
        assert torch.equal(e.pixels, full.pixels), (name, "pixels", where)
        assert torch.equal(e.image, full.image) and torch.equal(e.done, full.done), (name, "encodings", where)
        assert torch.equal(e.render_shadow(), ids), (name, "shadow", where)


def step_all(envs, actions, **kw):
    for e in envs:
        e.step(actions, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 31, 33, 65, 97, 24609])
def test_same_bytes_as_the_static_kernel(gpu, n):
    """12 steps of bench.py's action stream with auto-reset.  24 609 envs at one block per CU: 770 groups (the last one a single env), 385
    tickets over 256 blocks."""
    from babyai_amd.action_stream import actions_torch
    envs = trio(gpu, n, bpc=1 if n > 1000 else 0)
    acts = actions_torch(1234, 0, 12, 0, n, gpu)
    for t in range(12):
        step_all(envs, acts[t])
        same(*envs, where=(n, t))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [97, 2081])
def test_extreme_frames(gpu, n):
    """A step that changes nothing (every env holds: every mask is 0); the step after a reseed of every env (nearly every cell redrawn);
    steps in which exactly one env of every 32-env group moves (told to reset: a new level) and every other env holds."""
    import torch
    from babyai_amd.action_stream import actions_torch
    envs = trio(gpu, n, hold=True)
    new, old, full = envs
    acts = actions_torch(1234, 0, 8, 0, n, gpu)
    for t in range(3):
        step_all(envs, acts[t])
    same(*envs, where=(n, "warm"))
    before = new.pixels.clone()
    ids_before = new.render_shadow()
    step_all(envs, torch.full((n,), HOLD, dtype=torch.uint8, device=gpu))
    same(*envs, where=(n, "all hold"))
    assert torch.equal(new.pixels, before) and torch.equal(new.render_shadow(), ids_before)
    seeds = np.arange(n, dtype=np.uint64) * 7919 + 5
    for e in envs:
        e.reseed(None, seeds)
    step_all(envs, acts[3])
    same(*envs, where=(n, "after reseed"))
    changed = (new.render_shadow() != ids_before).any(dim=1).float().mean().item()
    assert changed > 0.9, changed                                         # (nearly every env was redrawn)
    for t in (4, 5):
        ids_before = new.render_shadow()
        one = torch.as_tensor([32 * g + (5 * g + t) % 32 for g in range((n + 31) // 32) if 32 * g + (5 * g + t) % 32 < n], dtype=torch.int64, device=gpu)
        step_all(envs, torch.full((len(one),), RESET_ENV, dtype=torch.uint8, device=gpu), ids=one)
        same(*envs, where=(n, "one env per group", t))
        dirty = (new.render_shadow() != ids_before).any(dim=1)
        listed = torch.zeros(n, dtype=torch.bool, device=gpu)
        listed[one] = True
        assert not bool((dirty & ~listed).any()) and int(dirty.sum()) > len(one) // 2, (n, t, int(dirty.sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("bpc", [3, 1])
@pytest.mark.parametrize("n", [33, 257])
def test_exact_footprint(gpu, n, bpc):
    """The registered buffer holds Q = 255 - (the new frame) before every step: afterwards exactly the 64-byte pieces that show a changed
    cell hold the new frame, every other byte is still Q, and the bands around the buffer are untouched."""
    import torch
    case = ru.CASE.get(n) or ru.Case(n, [12, 50, 31])
    ref = fp.Ref(gpu, False)
    a = fp.make_env(gpu, BOSS, n, pixel=True, seeds=41)
    b = fp.make_env(gpu, BOSS, n, seeds=41)                               # the same envs, no pixels: the encodings the steps must give
    fp.set_option(a, "render_delta_from_step", 1)
    fp.set_option(a, "render_delta_sched", 0)
    fp.set_option(a, "render_delta_bpc", bpc)
    fp.set_option(a, "render_piece_bytes", 64)
    for e in (a, b):
        fp.set_option(e, "consume_fused", 1)
        e.reset()
    target = fp.Target(a, gpu)
    acts = fp.step_actions(17, len(case.shifts), n, gpu)
    P = lambda x: ctypes.c_void_p(x.data_ptr())
    for k in range(len(case.shifts)):
        b.step(acts[k])
        new_enc = b.image.cpu().numpy()
        pat, kind = case.patterns(k)
        ru.check_patterns(pat, kind, **case.conditions(k))
        old_enc = ru.perturb(new_enc, pat, seed=k)
        old_ids, new_ids = ref.ids(old_enc), ref.ids(new_enc)
        fp.render(a, old_enc, target)                                     # the shadow: ids of the old frame; the step finds exactly the perturbed cells dirty
        assert a.get_option("render_delta_valid") == 1 and ref.same_ids(a.render_shadow(), old_ids)
        q = 255 - ref.flat_frames(new_ids)
        ref.put(target, q)
        assert a.lib.bbai_step_render(a.handle, P(acts[k]), P(a.image), P(a.direction), P(a.reward), P(a.reward64), P(a.done), 1, P(target.frame), a._stream()) == 0
        torch.cuda.synchronize()
        exp, mask = ref.expected(old_ids, new_ids, 64, q)
        assert ref.same(target, exp, mask, q), (n, bpc, k)
        assert torch.equal(a.image, b.image) and ref.same_ids(a.render_shadow(), new_ids), (n, bpc, k)
        assert target.bands_untouched(), (n, bpc, k)
    a.render_invalidate()


@pytest.mark.gpu
@pytest.mark.parametrize("split", [0, 1])
def test_ticket_counters_return_to_zero(gpu, split):
    """40 consecutive steps, every one compared with the full render: a ticket counter that a launch leaves above zero makes the next
    launch skip its first groups, a departure counter left above zero makes a later launch zero the tickets under running blocks (groups
    stored twice or never).  Split: two launches per step, the second one on envs 1024 .. 2080."""
    from babyai_amd.action_stream import actions_torch
    n = 2081
    envs = trio(gpu, n, split=split)
    acts = actions_torch(1234, 0, 40, 0, n, gpu)
    for t in range(40):
        step_all(envs, acts[t])
        same(*envs, where=(split, t))
