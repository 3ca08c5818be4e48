"""The handle's one owner (bbai_engine.hip: Owner) on the device: option "owned" counts what the handle holds -- device allocations, the pinned
words, streams, events -- and bbai_destroy releases exactly that, at whatever stage the handle is closed.

Two handles of 130 envs (two full 64-env blocks and a partial one), BBAI_LOOKAHEAD=2 (small rings):
  GoToLocal  in-place layout, lane generator, C plane
  GoTo       classic layout, window plane, lane-group generator
The expected numbers are written out by hand from the allocation sites of bbai_engine.hip -- never read back from the library."""
import numpy as np
import pytest

N = 130
SEED = 4100
STEPS = 20
LEVELS = ["BabyAI-GoToLocal-v0", "BabyAI-GoTo-v0"]

# bbai_create, by hand.  Both layouts: rec hot stale mt mti vhead vset pending first_slot win_meta totals flow gen_list gen_count (14), a plane
# + fcache (2: cplane in place, vplane classic), the lane generator's mtt mtpar lane_tmpl (3: both kinds are covered, the maze just does not
# use it by default), reset_list reset_slot counters atlas render_tickets lut (6), the pinned words (1); create_finish: the look-ahead and the
# split stream (2), ev_consumed ev_split0 ev_splitB ev_switch (4), ev_refill[NWIN = 34].  The ring: next_rec next_hot, + next_obs in place.
FRESH = {"BabyAI-GoToLocal-v0": 14 + 2 + 3 + 3 + 6 + 1 + 2 + 4 + 34, "BabyAI-GoTo-v0": 14 + 2 + 3 + 2 + 6 + 1 + 2 + 4 + 34}


@pytest.fixture(scope="module")
def small_rings():
    mp = pytest.MonkeyPatch()
    mp.setenv("BBAI_LOOKAHEAD", "2")
    for var in ("BBAI_INPLACE", "BBAI_VPLANE", "BBAI_CPLANE", "BBAI_PREGEN_LANE", "BBAI_LOOKAHEAD_STREAMS", "BABYAI_DONE_ACTIONS"):
        mp.delenv(var, raising=False)
    yield
    mp.undo()


def actions(gpu):
    import torch
    return torch.as_tensor(np.random.RandomState(9).randint(0, 7, size=(STEPS, N)).astype(np.uint8), device=gpu)


def run20(level, gpu):
    """A fresh handle stepped 20 times from the same seeds: every byte a caller sees, as one host array."""
    from babyai_amd.engine import BatchedBabyAIEnv
    env = BatchedBabyAIEnv(level, N, device=gpu, seeds=SEED)
    env.reset()
    out = [env.image.cpu().numpy().reshape(-1).copy(), env.direction.cpu().numpy().copy()]
    acts = actions(gpu)
    for t in range(STEPS):
        env.step(acts[t])
        out += [env.image.cpu().numpy().reshape(-1).copy(), env.direction.cpu().numpy().copy(), env.reward64.cpu().numpy().view(np.uint8).copy(),
                env.done.cpu().numpy().copy()]
    env.close()
    return np.concatenate(out)


@pytest.fixture(scope="module")
def reference(gpu, small_rings):
    """Computed once, by handles created (and closed) before any handle of these tests; never changed."""
    ref = {level: run20(level, gpu) for level in LEVELS}
    for r in ref.values():
        r.setflags(write=False)
    return ref


def use_every_lazy_path(env, gpu):
    """Every lazily allocated feature of a live handle, first use and second, with the increments of "owned" the allocation sites give."""
    import torch
    owned = lambda: env.get_option("owned")
    lib, h = env.lib, env.handle
    at = owned()

    def step_to(delta, what):
        nonlocal at
        at += delta
        assert owned() == at, what

    # bbai_set_render_target: rt_shadow + rt_dmask at the first registration; un-registering keeps both
    px = torch.zeros((N, 56, 56, 3), dtype=torch.uint8, device=gpu)
    assert lib.bbai_set_render_target(h, px.data_ptr()) == 0
    step_to(+2, "render target")
    assert lib.bbai_set_render_target(h, px.data_ptr()) == 0
    step_to(0, "render target, again")
    assert lib.bbai_set_render_target(h, None) == 0
    step_to(0, "render target un-registered: shadow and dirty masks stay")
    # bbai_step_tap_set: tap_mask tap_rank0 tap_perm tap_ids; a new list replaces them, an empty one frees them
    env.set_step_tap([0, 64, 129])
    step_to(+4, "tap set")
    env.set_step_tap([129, 1])
    step_to(0, "tap set, again")
    env.set_step_tap(None)
    step_to(-4, "tap cleared")
    env.set_step_tap([5, 128])
    step_to(+4, "tap set after clearing")
    # the expert's first decision (bot_alloc): bot_state bot_work bot_rows bot_stats
    env.bot_actions()
    step_to(+4, "first expert decision")
    env.bot_actions()
    step_to(0, "second expert decision")
    # an atlas + its lookup table per picture and tile size; a second installation reuses both
    for picture, sizes in (("grid", (8, 16, 32)), ("view", (16, 32))):
        for ts in sizes:
            env._install_atlas(picture, ts)
            step_to(+2, "%s atlas at %d" % (picture, ts))
        for ts in sizes:
            env._atlases.discard((picture, ts))
            env._install_atlas(picture, ts)
            step_to(0, "%s atlas at %d, again" % (picture, ts))
    # done-action mode: lsm
    for enable, delta in ((1, +1), (1, 0), (0, -1), (0, 0)):
        assert lib.bbai_set_done_actions(h, enable) == 0
        step_to(delta, "done actions %d" % enable)
    # the first bbai_reseed (reseed_scratch): rs_list rs_count rs_pending rs_first rs_claim, ev_rs_call ev_rs_done, ev_rs_part[1..7]
    env.reseed([3, 70], [5, 6])
    step_to(+5 + 2 + 7, "first reseed")
    env.reseed([129], [7])
    step_to(0, "second reseed")
    # set_sides: 1 -> 2 makes sides[1], gen_lists[1], gen_counts[1], mark_stream, ev_part[0], ev_part[1]; 2 -> 1 destroys the two streams and
    # keeps the lists and the events, so going up again only makes the streams again
    for want, delta in ((2, +6), (2, 0), (1, -2), (1, 0), (2, +2)):
        env.set_option("lookahead_streams", want)
        step_to(delta, "lookahead_streams -> %d" % want)
    # bbai_profile: an event pair per ring slot a bracketed launch has used.  With the consume fused into k_step an encoded step is ONE bracketed
    # launch; the ring (256 slots per kernel) goes on where it stood, so a second profiled stretch uses three NEW slots.
    env.set_option("consume_fused", 1)
    acts = actions(gpu)
    env.profile(True)
    for t in range(3):
        env.step(acts[t])
    step_to(+2 * 3, "three profiled steps")
    env.profile_pause()
    for t in range(3):
        env.step(acts[t])
    step_to(0, "steps without the profile")
    env.profile_resume()
    for t in range(3):
        env.step(acts[t])
    step_to(+2 * 3, "three more profiled steps")
    env.profile_pause()
    return px


@pytest.mark.gpu
@pytest.mark.parametrize("level", LEVELS)
def test_owned_counts_what_the_allocation_sites_say(gpu, small_rings, level):
    from babyai_amd.engine import BatchedBabyAIEnv
    env = BatchedBabyAIEnv(level, N, device=gpu)
    single = level == "BabyAI-GoToLocal-v0"
    assert env.get_option("lookahead_period") == 2 and env.get_option("lookahead_streams") == 1
    assert (env.get_option("inplace"), env.get_option("cplane"), env.get_option("pregen_lane")) == ((1, 1, 1) if single else (0, 0, 0))
    assert env.get_option("owned") == FRESH[level]
    env.seed(SEED)
    assert env.get_option("owned") == FRESH[level], "bbai_seed's staged seeds die with the call"
    env.reset()
    rec, hot, stale = env.export_state()
    env.import_state(rec, hot, stale)
    assert env.get_option("owned") == FRESH[level], "bbai_import_state's staged hot states die with the call"
    keep = use_every_lazy_path(env, gpu)
    env.close()
    del keep


@pytest.mark.gpu
@pytest.mark.parametrize("stage", ["never_seeded", "seeded_never_reset", "every_lazy_path_then_20_steps"])
@pytest.mark.parametrize("level", LEVELS)
def test_close_at_every_stage(gpu, small_rings, reference, level, stage):
    """close() returns at every stage of a handle's life, and a handle created afterwards computes what one created before did."""
    from babyai_amd.engine import BatchedBabyAIEnv
    env = BatchedBabyAIEnv(level, N, device=gpu)
    keep = None
    if stage != "never_seeded":
        env.seed(SEED)
    if stage == "every_lazy_path_then_20_steps":
        env.reset()
        keep = use_every_lazy_path(env, gpu)
        acts = actions(gpu)
        for t in range(STEPS):
            env.step(acts[t])
        assert env.gate_timeouts() == 0
    env.close()
    assert not env.handle
    del keep
    assert np.array_equal(run20(level, gpu), reference[level])
