"""The batched expert (babyai_amd/csrc/bbai_bot.hpp, host build) against decisions recorded from the reference's
own babyai/bot.py (tests/golden/bot/*.npz, made by tools/gen_golden_bot.py): every suggestion, in pure mode and in
advised mode (12 % random actions, the bot is told), including the step at which the reference bot gives up."""
import glob
import os

import numpy as np
import pytest

from babyai_amd.levels import make_cfg
from hostsim_util import HostBot, HostEnv

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "bot", "*.npz")))


def replay(path, mode):
    with np.load(path) as f:
        g = {k: f[k] for k in f.files}
    name = str(g["level"])
    suggest, action, done = g[mode + "_suggest"], g[mode + "_action"], g[mode + "_done"]
    n_steps, n_envs = suggest.shape
    mismatches = []
    capacity = 0
    for i in range(n_envs):
        env = HostEnv(make_cfg(name), int(g["seed_base"]) + i)
        env.reset()
        bot = HostBot(env)
        first, last, alive = True, None, True
        for t in range(n_steps):
            if alive:
                a = bot.decide(first, last)
                first = False
                want = int(suggest[t, i])
                if a is None and bot.dead_reason == 2:
                    capacity += 1
                if (a if a is not None else -1) != want:
                    mismatches.append((name, mode, i, t, a, want))
                    break
                alive = a is not None
            else:
                assert suggest[t, i] == -1
            last = int(action[t, i])
            _, _, d = env.step(last)
            assert bool(d) == bool(done[t, i]), (name, mode, i, t)
            if d:
                env.reset()
                first, last, alive = True, None, True
    return mismatches, capacity


@pytest.fixture(params=[0, 1], ids=["lazy-search", "eager-search"])
def eager(request):
    """The first search tree expanded inside the queries (0) or to exhaustion at the top of every decision (1, the
    device default): same tree, same pop order, so the decisions must not change."""
    from hostsim_util import lib
    lib().hs_bot_set_eager(request.param)
    yield request.param
    lib().hs_bot_set_eager(0)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
@pytest.mark.parametrize("mode", ["pure", "advised"])
def test_bot_decisions_match_reference(path, mode, eager):
    mismatches, capacity = replay(path, mode)
    assert not mismatches, mismatches[:3]
    # A death by capacity (subgoal stack full) that the reference shares is the reference bot replanning for ever
    # (2 s decision budget in tools/gen_golden_bot.py): only UnlockToUnlock does that.
    assert capacity == 0 or "UnlockToUnlock" in path


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_find_obj_pos_shortcut_equals_the_packed_lists(path):
    """bbai_bot.hpp's _find_obj_pos pairs every object with its own position, position key as loop order, when every object of
    the descriptor is still recorded where the episode started it -- equivalent to zip(obj_set, obj_poss) only because the start
    positions are distinct and nothing of the set has moved.  Property test: the shortcut switched OFF (every query through the two
    sorted lists), every reference-bot fixture with its 20 % random actions (carried, dropped, stale objects) must replay to the same
    decisions as with it ON (test_bot_decisions_match_reference)."""
    from hostsim_util import lib
    lib().hs_bot_set_aligned(0)
    lib().hs_bot_set_eager(1)
    try:
        for mode in ("pure", "advised"):
            mismatches, _ = replay(path, mode)
            assert not mismatches, (mode, mismatches[:3])
    finally:
        lib().hs_bot_set_aligned(1)
        lib().hs_bot_set_eager(0)


WIDTH_LEVELS = ("BossLevel", "SynthSeq", "KeyCorridorS6R3", "UnlockToUnlock", "PutNextS7N4Carrying", "BlockedUnlockPickup", "GoToImpUnlock",
                "PickupDist", "MoveTwoAcrossS8N9", "GoToLocal")


def _lanes(n):
    from hostsim_util import lib
    lib().hs_bot_set_lanes(n)
    lib().hs_bot_set_eager(1)


def _one_lane():
    from hostsim_util import lib
    lib().hs_bot_set_lanes(1)
    lib().hs_bot_set_eager(0)


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_lane_group_decisions_match_reference(path):
    """The lane-group form of the expert (k_botg on the device: 16 lanes per env), its lanes emulated as fibers that run one at a time
    between the group's collectives (tests/hostsim/hostsim.cpp EmuGroup): the 49 view cells, the mask rows, the four neighbours of a
    popped position, the acceptance scans and the key scan split over the lanes -- same decisions, or the group form is wrong.
    (a = -3 / -4 in a mismatch: the emulator saw the lanes diverge around a collective / disagree on the decision.)"""
    _lanes(16)
    try:
        # (advised: 12 % random actions, so the undo logic runs too; the levels with the longest plans also in pure mode)
        for mode in ("advised", "pure") if os.path.basename(path)[:-4] in WIDTH_LEVELS else ("advised",):
            mismatches, capacity = replay(path, mode)
            assert not mismatches, (mode, mismatches[:3])
            assert capacity == 0 or "UnlockToUnlock" in path
    finally:
        _one_lane()


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("lanes", [4, 32])
@pytest.mark.parametrize("level", WIDTH_LEVELS)
def test_lane_group_width_does_not_matter(level, lanes):
    """Other group widths (chunking of the scans, 4 = every lane expands a neighbour) on the levels with the longest plans."""
    path = os.path.join(HERE, "golden", "bot", level + ".npz")
    _lanes(lanes)
    try:
        mismatches, _ = replay(path, "advised")
        assert not mismatches, mismatches[:3]
    finally:
        _one_lane()


DIFFERENTIAL = [("BossLevel", 24, 300), ("SynthSeq", 16, 200), ("KeyCorridorS6R3", 8, 250)]
SWITCH_ON = ["GoToLocal", "PickupLoc", "GoTo", "Unlock"]


def _reference(key):
    """The reference's answers to one of these protocols (tests/refpin_util.Replay over tools/gen_golden_refpin.py's record)."""
    import refpin_util as rp
    return rp.Replay(rp.load_json("bot_reference.json.gz")[key])


def _differential(ref, level, n_envs, steps):
    """Seeds not in the fixtures above, the reference's Bot next to the host build, 8 % random actions in between."""
    rng = np.random.RandomState(len(level))
    checked = 0
    for i in range(n_envs):
        seed = 880000 + 37 * i
        ref.make(level, seed, "seed")
        env = HostEnv(make_cfg(level), seed)
        env.reset()
        ref.new_bot()
        hbot = HostBot(env)
        first, last = True, None
        for t in range(steps):
            want = ref.replan(last, 3.0)
            got = hbot.decide(first, last)
            first = False
            assert got == want, (level, seed, t, got, want)
            checked += 1
            if want is None:
                break
            a = want if rng.rand() > 0.08 else int(rng.randint(0, 7))
            last = a
            r, d = ref.step(a)
            _, hr, hd = env.step(a)
            assert bool(d) == bool(hd) and np.float32(r) == hr
            if d:
                ref.reset()
                env.reset()
                ref.new_bot()
                hbot = HostBot(env)
                first, last = True, None
    assert checked > n_envs * steps // 2


@pytest.mark.timeout(900)
@pytest.mark.parametrize("level,n_envs,steps", DIFFERENTIAL)
def test_bot_differential_against_live_reference(level, n_envs, steps):
    """Fresh seeds (not in the fixtures of the tests above): what the reference's Bot decided, live, when
    tools/gen_golden_refpin.py ran this protocol, against the host build."""
    ref = _reference("differential/%s" % level)
    _differential(ref, level, n_envs, steps)
    assert ref.finished()


def _stack_capacity(ref):
    level, seed = "MiniBossLevel", 520
    env = HostEnv(make_cfg(level), seed)
    env.reset()
    bot = HostBot(env)                      # default capacity
    deep_env = HostEnv(make_cfg(level), seed)
    deep_env.reset()
    deep = HostBot(deep_env, stack_cap=1024)
    ref.make(level, seed, "ctor")
    ref.new_bot()
    first, t, done, reward, deepest = True, 0, False, 0.0, 0
    while not done:
        b = deep.decide(first, None)
        assert b is not None, t
        deepest = max(deepest, deep.stack_depth)
        if t <= 63:
            a = bot.decide(first, None)
            assert (a == b) if t < 63 else (a is None and bot.dead_reason == 2), t
            if t < 63:
                env.step(a)
        want, depth = ref.replan(), ref.stack_depth()
        assert want == b and depth == deep.stack_depth, t
        ref.step(b)
        first = False
        _, reward, done = deep_env.step(b)
        t += 1
    assert reward == 0 and t == deep_env.max_steps and deepest > 48


def test_stack_capacity_is_the_one_documented_divergence():
    """MiniBossLevel, `Level(seed=520)`: the reference bot enters an unproductive loop that grows its subgoal stack by
    about four entries every five steps and keeps acting until max_steps (episode failed, reward 0).  With the default
    48-entry stack the port reports 'gave up' (reason = capacity) at step 63, where the reference's stack reaches 52;
    with a deeper stack (BBAI_BOT_STACK / stack_cap) it follows the reference to the end of the episode.
    Either way the episode fails; demonstrations (first SOLVED episode per stream) are unaffected.  The reference's decisions and
    stack depths: tools/gen_golden_refpin.py's record."""
    ref = _reference("stack_capacity")
    _stack_capacity(ref)
    assert ref.finished()


def _switch_on(ref, level):
    rng = np.random.RandomState(3)
    for k in range(6):
        seed = 990000 + k
        ref.make(level, seed, "seed_keep")
        env = HostEnv(make_cfg(level), seed)
        env.reset()
        hbot = HostBot(env)
        for _ in range(2):                                   # two switch-on points per mission
            done = False
            for t in range(int(rng.randint(3, 12))):
                a = int(rng.choice([0, 1, 2]))
                _, d = ref.step(a)
                env.step(a)
                if d:
                    done = True
                    break
            if done:
                break
            ref.new_bot()
            last = None
            for t in range(40):
                want = ref.replan(last)
                got = hbot.decide(False, last)               # no `first` flag: the port notices by itself
                assert got == want, (level, seed, t)
                last = want
                _, d = ref.step(want)
                env.step(want)
                if d or t == 12:
                    done = d
                    break
            if done:
                break


@pytest.mark.parametrize("level", SWITCH_ON)
def test_expert_switched_on_mid_episode(level):
    """`Bot(env)` constructed in the middle of an episode (after random steps) vs the port, which starts a fresh plan by
    itself when it was not consulted on the previous step.  Only turn/forward noise before the switch, so that no
    described object has moved (see bot_decide).  The reference's side: tools/gen_golden_refpin.py's record."""
    ref = _reference("switch_on/%s" % level)
    _switch_on(ref, level)
    assert ref.finished()