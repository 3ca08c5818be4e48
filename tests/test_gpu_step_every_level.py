"""The step kernels (k_step, k_step_ticks) on every registered level, held env by env and byte by byte to the host build of the same
headers (tests/hostsim_util.py HostBatch, which tests/test_hostsim_batch.py pins to the per-env host build), at 1 024 envs, with a
closed-loop expert policy so that episodes really end in success, failure, timeout and reset commands -- and a scattered sample
straight against the Python oracle.  The generator got this net in tests/test_gpu_lane_generator.py after a compiler fault showed up in
3 of 1 024 envs and 2 of 105 level kinds; the step kernels are built by the same compiler with the same flags.

  (a) test_per_step_every_level          every level, default layout: per-step calls (k_step), the expert's suggestions with 6 % random
                                          actions, 0.3 % reset commands (action 7); every output of every env every step, the exported
                                          state every 25 steps; 32 scattered envs also against the oracle (spawned workers, no GPU)
  (b)   ... same test, second half       the recorded actions replayed through bbai_rollout with the stepping lanes' tap on every env:
                                          k_step_ticks (several steps per launch) against the host results of (a)
  (c) test_every_instantiation           (a) + (b) on eight levels under every state layout / consume mode / auto-reset setting
  (d) test_done_actions_every_level      the done-action verifier mode on every level, with and without the enum rule
  (e) test_timeouts_on_the_large_levels  multi-room episodes run past max_steps (rollout, turning in place)

Which of the 12 kernels each test launches, <VP, FUSE, CP> (the step path bbai_engine.hip step_kernel picks):

  kernel (k_step and k_step_ticks)   layout                       reached by
  <false, 3, true>                   in place, C plane            (a)/(b) single rooms; (c) inplace, frozen_inplace; (d) single rooms
  <false, 3, false>                  in place, no C plane         (c) inplace_nocplane, frozen_inplace_nocplane, inplace on a maze
  <true, 1, false>                   classic, window plane, fused (a)/(b) mazes; (c) classic_fused; (d)/(e) mazes
  <false, 1, false>                  classic, record only, fused  (c) novplane_fused
  <true, 0, false>                   classic, window plane        (c) classic_unfused (k_step only: an unfused auto-reset keeps one step
                                                                  per launch), frozen_classic (both)
  <false, 0, false>                  classic, record only         (c) novplane_unfused (k_step), frozen_novplane (both)

test_zz_every_instantiation_was_launched checks that the run reached all twelve, and prints the episode endings per level."""
import collections
import multiprocessing

import numpy as np
import pytest

from babyai_amd.levels import LEVELS, make_cfg

ALL = sorted(LEVELS)
SUBSET = ["GoToLocal", "PickupLoc", "GoTo", "BossLevel", "PutNextS5N2Carrying", "KeyInBox", "SynthS5R2", "UnlockToUnlock"]
N, T, STATE_EVERY, ORACLE_ENVS = 1024, 200, 25, 32
CUTS = [0, 5, 6, 45, 150, T]        # rollout calls that end and start in mid-window, ones that span several windows, a one-step call
RESET_ENV = 7
# (env variables at bbai_create, options set after it, auto_reset)
VARIANTS = {
    "inplace": ({"BBAI_INPLACE": "1"}, {}, True),
    "inplace_nocplane": ({"BBAI_INPLACE": "1", "BBAI_CPLANE": "0"}, {}, True),
    "classic_fused": ({"BBAI_INPLACE": "0"}, {"consume_fused": 1}, True),
    "classic_unfused": ({"BBAI_INPLACE": "0"}, {"consume_fused": 0}, True),
    "novplane_fused": ({"BBAI_INPLACE": "0", "BBAI_VPLANE": "0"}, {"consume_fused": 1}, True),
    "novplane_unfused": ({"BBAI_INPLACE": "0", "BBAI_VPLANE": "0"}, {"consume_fused": 0}, True),
    "frozen_inplace": ({"BBAI_INPLACE": "1"}, {}, False),
    "frozen_inplace_nocplane": ({"BBAI_INPLACE": "1", "BBAI_CPLANE": "0"}, {}, False),
    "frozen_classic": ({"BBAI_INPLACE": "0"}, {}, False),
    "frozen_novplane": ({"BBAI_INPLACE": "0", "BBAI_VPLANE": "0"}, {}, False),
}
ENDS = collections.defaultdict(collections.Counter)       # level -> how the episodes of (a) ended
LAUNCHED = set()                                          # (kernel, <VP, FUSE, CP>) the tests saw launched
DONE_ENDS = collections.Counter()                         # ... and of (d)


# ---- the oracle side (worker processes: spawned, they never touch the GPU) ----------------------------------------------------
def _oracle_run(args):
    """Oracle envs of `seeds` stepped with acts[t, k] as the engine steps an auto-resetting env (7 = reset this env) -> images [T + 1, k, 7, 7, 3],
    directions [T + 1, k], rewards (f64) [T, k], dones [T, k]."""
    from oracle import levels as olevels
    level, seeds, acts = args
    envs = []
    for s in seeds:
        e = olevels.make_env(level)
        e.seed(int(s))
        envs.append(e)
    cur = [e.reset() for e in envs]
    steps, k = acts.shape
    img = np.zeros((steps + 1, k, 7, 7, 3), np.uint8)
    dirs = np.zeros((steps + 1, k), np.uint8)
    rew = np.zeros((steps, k), np.float64)
    done = np.zeros((steps, k), np.uint8)
    for j in range(k):
        img[0, j], dirs[0, j] = cur[j]["image"], cur[j]["direction"]
    for t in range(steps):
        for j, e in enumerate(envs):
            a = int(acts[t, j])
            if a == RESET_ENV:
                o, r, d = None, 0.0, True
            else:
                o, r, d, _ = e.step(a)
            if d:
                o = e.reset()
            rew[t, j], done[t, j] = r, d
            img[t + 1, j], dirs[t + 1, j] = o["image"], o["direction"]
    return img, dirs, rew, done


@pytest.fixture(scope="module")
def oracle_pool():
    pool = multiprocessing.get_context("spawn").Pool(4)
    yield pool
    pool.terminate()
    pool.join()


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def _make(gpu, level, n, seed, monkeypatch, env_vars=(), opts=(), auto_reset=True, done_actions=None):
    from babyai_amd.engine import BatchedBabyAIEnv
    with monkeypatch.context() as m:
        for k, v in dict(env_vars).items():
            m.setenv(k, v)
        env = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device=gpu, seeds=seed, auto_reset=auto_reset, done_actions=done_actions)
    for k, v in dict(opts).items():
        env.set_option(k, v)
        assert env.get_option(k) == v, k
    return env


def _instantiation(env, env_vars, auto_reset):
    """<VP, FUSE, CP> of the step kernel this handle launches (bbai_engine.hip step_kernel), from what it reports about itself."""
    c = env.cfg
    if env.get_option("inplace"):
        return (False, 3, bool(env.get_option("cplane")))
    cf = env.get_option("consume_fused")
    fused = auto_reset and (cf == 1 or (cf == -1 and c.num_rows * c.num_cols > 1))
    return (dict(env_vars).get("BBAI_VPLANE") != "0", 1 if fused else 0, False)


def _diff(what, level, t, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if np.array_equal(got, want):
        return
    bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
    raise AssertionError("%s: %s differs at step %s in %d envs, first %s" % (level, what, t, len(bad), bad[:8].tolist()))


def _outputs(env):
    return (env.image.cpu().numpy(), env.direction.cpu().numpy(), env.reward.cpu().numpy(), env.reward64.cpu().numpy(), env.done.cpu().numpy())


def _check_outputs(level, t, env, host):
    img, dirs, rew, rew64, done = _outputs(env)
    _diff("image", level, t, img, host.image)
    _diff("direction", level, t, dirs, host.direction)
    _diff("reward f32 bits", level, t, rew.view(np.uint32), host.reward.view(np.uint32))
    _diff("reward f64 bits", level, t, rew64.view(np.uint64), host.reward64.view(np.uint64))
    _diff("done", level, t, done, host.done)


def _check_state(level, t, env, host):
    rec, hot, stale = env.export_state()
    _diff("record", level, t, rec, host.rec)
    _diff("hot bytes 0..14", level, t, hot[:, :15], host.hot[:, :15])      # (byte 15: the env's ring slot, bookkeeping only)
    _diff("stale set", level, t, stale, host.stale)


def _closed_loop(gpu, level, env, host, steps, seed, ends=None, state_every=STATE_EVERY):
    """Steps env (per-step calls) and host with the device expert's suggestions, ~6 % random actions, ~0.3 % reset commands and a random action
    where the bot gave up; compares every output every step and the state every `state_every` steps.  Returns the actions uint8[steps, n] and the
    host's outputs after every step (image, direction, reward64, done)."""
    import torch
    n = env.num_envs
    rng = np.random.RandomState(seed)
    env.reset()
    host.reset()
    _diff("first image", level, -1, env.image.cpu().numpy(), host.image)
    _diff("first direction", level, -1, env.direction.cpu().numpy(), host.direction)
    acts = np.zeros((steps, n), np.uint8)
    log = {"image": np.zeros((steps, n, 7, 7, 3), np.uint8), "direction": np.zeros((steps, n), np.uint8),
           "reward64": np.zeros((steps, n), np.float64), "done": np.zeros((steps, n), np.uint8)}
    prev = None
    for t in range(steps):
        sug = env.bot_actions(prev).cpu().numpy()
        u = rng.rand(n)
        a = np.where((sug == env.BOT_GAVE_UP) | (u < 0.06), rng.randint(0, 7, n), sug).astype(np.uint8)
        a[u > 0.997] = RESET_ENV
        acts[t] = a
        live = host.hot[:, 13] == 0
        step_after = host.step_count + 1
        max_steps = host.max_steps
        prev = torch.as_tensor(a, device=gpu)
        env.step(prev)
        host.step(a)
        _check_outputs(level, t, env, host)
        if (t + 1) % state_every == 0 or t == steps - 1:
            _check_state(level, t, env, host)
        for k in log:
            log[k][t] = getattr(host, k)
        if ends is not None:
            fin = live & (host.done == 1)
            ends["reset"] += int((fin & (a == RESET_ENV)).sum())
            fin &= a != RESET_ENV
            ends["success"] += int((fin & (host.reward64 > 0)).sum())
            fin &= host.reward64 == 0
            ends["timeout"] += int((fin & (step_after >= max_steps)).sum())
            ends["failure"] += int((fin & (step_after < max_steps)).sum())
    return acts, log


def _replay_ticks(gpu, level, env, acts, log, host, expect_multi, cuts=CUTS):
    """The recorded actions through bbai_rollout with the stepping lanes logging EVERY env (set_step_tap): k_step_ticks where the window allows
    several steps per launch.  Every logged row against the host's outputs of the same step, then the state the run leaves."""
    import torch
    steps, n = acts.shape
    env.reset()
    env.set_step_tap(list(range(n)))
    tap = {"image": torch.zeros((steps, n, 7, 7, 3), dtype=torch.uint8, device=gpu), "direction": torch.zeros((steps, n), dtype=torch.uint8, device=gpu),
           "reward64": torch.zeros((steps, n), dtype=torch.float64, device=gpu), "done": torch.zeros((steps, n), dtype=torch.uint8, device=gpu)}
    dacts = torch.as_tensor(acts, device=gpu)
    env.profile(True)
    for t0, t1 in zip(cuts, cuts[1:]):
        env.rollout(dacts[t0:t1], tap=tap, obs_row0=t0, row0=t0, step_tap=True)
    launches = env.profile_read()["k_step"][1]
    ticks = env.get_option("profile_step_ticks")
    env.profile(False)
    got = {k: v.cpu().numpy() for k, v in tap.items()}
    for t in range(steps):
        _diff("rollout image", level, t, got["image"][t], log["image"][t])
        _diff("rollout direction", level, t, got["direction"][t], log["direction"][t])
        _diff("rollout reward f64 bits", level, t, got["reward64"][t].view(np.uint64), log["reward64"][t].view(np.uint64))
        _diff("rollout done", level, t, got["done"][t], log["done"][t])
    _check_outputs(level, steps - 1, env, host)
    _check_state(level, steps - 1, env, host)
    assert ticks == steps, (level, ticks, steps)
    if expect_multi:
        assert launches < ticks, "%s: %d k_step launches for %d steps: the multi-tick path did not run" % (level, launches, ticks)
    return launches < ticks


def _run(gpu, level, monkeypatch, variant=None, oracle_pool=None, seed=20000):
    from hostsim_util import HostBatch
    env_vars, opts, auto = VARIANTS[variant] if variant else ({}, {}, True)
    seeds = np.arange(seed, seed + N)
    a = _make(gpu, level, N, seed, monkeypatch, env_vars, opts, auto)
    kern = _instantiation(a, env_vars, auto)
    for k, v in env_vars.items():      # the intended variant is the one that runs
        if k == "BBAI_INPLACE":
            assert a.get_option("inplace") == int(v), (level, variant)
        if k == "BBAI_CPLANE":
            assert a.get_option("cplane") == 0, (level, variant)
    host = HostBatch(make_cfg(level), seeds, auto_reset=auto)
    ends = ENDS[level] if variant is None else None
    acts, log = _closed_loop(gpu, level, a, host, T, seed=len(level) + 7 * len(variant or ""), ends=ends)
    assert a.generator_failures() == 0
    a.close()
    LAUNCHED.add(("k_step", kern))
    pending = None
    if oracle_pool is not None:
        from babyai_amd.shard import scattered_ids
        ids = np.asarray(scattered_ids(N, ORACLE_ENVS))
        parts = np.array_split(ids, 4)
        pending = (ids, oracle_pool.map_async(_oracle_run, [(level, [int(seeds[i]) for i in p], acts[:, p]) for p in parts]))
    # (b): the same trajectories through the rollout entry
    b = _make(gpu, level, N, seed, monkeypatch, env_vars, opts, auto)
    assert _instantiation(b, env_vars, auto) == kern
    host = HostBatch(make_cfg(level), seeds, auto_reset=auto)
    host.reset()
    for t in range(T):
        host.step(acts[t])
    expect_multi = kern[1] != 0 or not auto        # (an unfused auto-reset keeps one step per launch: k_consume runs between the steps)
    if _replay_ticks(gpu, level, b, acts, log, host, expect_multi):
        LAUNCHED.add(("k_step_ticks", kern))
    b.close()
    if pending is not None:
        ids, res = pending
        out = res.get(timeout=600)
        img, dirs, rew, done = (np.concatenate([o[k] for o in out], axis=1) for k in range(4))
        for t in range(T):
            _diff("image vs oracle (env = index into the scattered sample)", level, t, log["image"][t][ids], img[t + 1])
            _diff("direction vs oracle", level, t, log["direction"][t][ids], dirs[t + 1])
            _diff("reward f64 bits vs oracle", level, t, log["reward64"][t][ids].view(np.uint64), rew[t].view(np.uint64))
            _diff("done vs oracle", level, t, log["done"][t][ids], done[t])
    return kern


# ---- (a) + (b) + (f): every level, default layout -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("level", ALL)
def test_per_step_every_level(gpu, level, monkeypatch, oracle_pool):
    _run(gpu, level, monkeypatch, oracle_pool=oracle_pool)
    e = ENDS[level]
    assert e["success"] > 0, (level, dict(e))
    assert e["reset"] > 0, (level, dict(e))


# ---- (c): every instantiation --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("level", SUBSET)
def test_every_instantiation(gpu, level, variant, monkeypatch):
    _run(gpu, level, monkeypatch, variant=variant, seed=30000)


# ---- (d): the done-action verifier mode ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("enum_done", [0, 1])
@pytest.mark.parametrize("level", ALL)
def test_done_actions_every_level(gpu, level, enum_done, monkeypatch):
    """BABYAI_DONE_ACTIONS (include/bbai.h bbai_set_done_actions): the expert's `done` after each completed instruction is what succeeds;
    with option done_action_enum 1 the AndInstr identity rule runs (hs_step64_done_enum on the host)."""
    from hostsim_util import HostBatch
    n, seed = 256, 40000
    env = _make(gpu, level, n, seed, monkeypatch, done_actions=True)
    assert env.done_actions
    if enum_done:
        env.set_option("done_action_enum", 1)
    assert env.get_option("done_action_enum") == enum_done
    host = HostBatch(make_cfg(level), np.arange(seed, seed + n), done_actions=True, enum_done=bool(enum_done))
    ends = collections.Counter()
    _closed_loop(gpu, level, env, host, 150, seed=3 + enum_done, ends=ends, state_every=50)
    assert env.generator_failures() == 0
    LAUNCHED.add(("k_step", _instantiation(env, {}, True)))
    env.close()
    DONE_ENDS.update(ends)


# ---- (e): timeouts on the large levels -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("level", ["GoTo", "GoToObjMaze", "MiniBossLevel"])
def test_timeouts_on_the_large_levels(gpu, level, monkeypatch):
    """Turning in place for longer than max_steps: the episodes of a maze end by timeout (a GoTo whose target starts next to the agent may
    still succeed), every step of every env against the host, through the rollout entry."""
    from hostsim_util import HostBatch
    n, seed = 256, 50000
    host = HostBatch(make_cfg(level), np.arange(seed, seed + n))
    host.reset()
    steps = int(host.max_steps.max()) + 40
    rng = np.random.RandomState(5)
    acts = rng.randint(0, 2, (steps, n)).astype(np.uint8)           # left / right only
    log = {"image": np.zeros((steps, n, 7, 7, 3), np.uint8), "direction": np.zeros((steps, n), np.uint8),
           "reward64": np.zeros((steps, n), np.float64), "done": np.zeros((steps, n), np.uint8)}
    timeouts = 0
    for t in range(steps):
        step_after = host.step_count + 1
        max_steps = host.max_steps
        host.step(acts[t])
        timeouts += int(((host.done == 1) & (host.reward64 == 0) & (step_after >= max_steps)).sum())
        for k in log:
            log[k][t] = getattr(host, k)
    assert timeouts > n // 2, (level, timeouts)
    env = _make(gpu, level, n, seed, monkeypatch)
    kern = _instantiation(env, {}, True)
    cuts = [0, 7, 8, 300, steps]
    if _replay_ticks(gpu, level, env, acts, log, host, kern[1] != 0, cuts=cuts):
        LAUNCHED.add(("k_step_ticks", kern))
    env.close()


# ---- what the run reached ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_zz_every_instantiation_was_launched(gpu):
    """After the tests above (file order): the twelve kernels were all launched, and the per-level episode endings of (a) -- printed -- show
    failures as a visible share, not zero."""
    if len(ENDS) < len(ALL) or not LAUNCHED:
        pytest.skip("runs after the whole file only (%d of %d levels ran)" % (len(ENDS), len(ALL)))
    tot = collections.Counter()
    for level in ALL:
        e = ENDS[level]
        tot.update(e)
        print("ENDS %-28s success %6d failure %6d timeout %6d reset %6d" % (level, e["success"], e["failure"], e["timeout"], e["reset"]))
    print("ENDS total", dict(tot), "done-action mode", dict(DONE_ENDS))
    for k in sorted(LAUNCHED):
        print("LAUNCHED", k[0], "<%s, %d, %s>" % (str(k[1][0]).lower(), k[1][1], str(k[1][2]).lower()))
    want = {(k, (vp, f, cp)) for k in ("k_step", "k_step_ticks") for vp, f, cp in
            [(False, 3, True), (False, 3, False), (True, 1, False), (False, 1, False), (True, 0, False), (False, 0, False)]}
    assert want <= LAUNCHED, sorted(want - LAUNCHED)
    assert tot["failure"] > 0.01 * sum(tot.values()), dict(tot)
    assert DONE_ENDS["success"] > 0 and DONE_ENDS["failure"] > 0, dict(DONE_ENDS)
