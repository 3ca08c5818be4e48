"""SHORT reseeds on the device (include/bbai.h bbai_reseed with option "reseed_levels"; BatchedBabyAIEnv.reseed(ids, seeds, levels=k)): a listed env
gets k levels of its seed's stream instead of a whole look-ahead ring and PARKS -- frozen -- when the k-th ends.  n = 192 envs, 37 listed (0, n - 1 and
both sides of every 64-env boundary among them), BBAI_LOOKAHEAD = 4 but for one default-period case.

  1. the option by name (the test that fails without the feature: "unknown option");
  2. the scripted runs of tests/reseed_levels_util.py -- depths 1, 2, 3, the ring's depth and 5 beyond it; reseeds in front of window positions 0, 2
     and 3; envs that spend their levels inside one window; parked envs reseeded at depth 1 and at depth 0; auto_reset=False with one reset() -- under
     env.step with token rows, the many-ticks launch of rollout(), pixel steps (bbai_step_render) and bot_rollout, on five state layouts, against the
     host model that parks and against a TWIN handle that gets the same reseeds at depth 0: every byte of every unlisted env equals the twin's at
     every step; every byte of a listed env equals the model's and the twin's until it parks; while parked its done is 1, its reward unchanged, the
     expert answers 6, and image / direction / token row are not compared;
  3. a checkpoint with parked and half-spent envs continues identically in a fresh handle;
  4. evaluate_policy(pool=64, reseed_levels=1) logs what pool=64 and the default path log;
  5. collect_seeds(reseed_levels=1) returns the default's (store, kept).
Every handle ends with gate_timeouts == 0 and generator_failures() == 0."""
import numpy as np
import pytest

import reseed_levels_util as rl
import scenario_util as su

B, RING, N = rl.B, rl.RING, 192
G, BOSS = "GoToLocal", "BossLevel"
IP1, IP0 = {"BBAI_INPLACE": "1"}, {"BBAI_INPLACE": "0"}
IP0F = {"BBAI_INPLACE": "0", "BBAI_CONSUME_FUSED": "1"}
IP0U = {"BBAI_INPLACE": "0", "BBAI_CONSUME_FUSED": "0"}
LANE0 = {"BBAI_INPLACE": "1", "BBAI_PREGEN_LANE": "0"}


@pytest.fixture(autouse=True)
def _short_windows(monkeypatch):
    monkeypatch.setenv("BBAI_LOOKAHEAD", str(B))


def _id(*parts):
    return "-".join("-".join("%s%s" % (k[5:].lower(), v) for k, v in sorted(p.items())) if isinstance(p, dict) else str(p) for p in parts)


def _make(gpu, monkeypatch, sc, ev, tokens=False, period=B, **kw):
    from babyai_amd.engine import BatchedBabyAIEnv
    for k, v in ev.items():
        monkeypatch.setenv(k, v)
    env = BatchedBabyAIEnv("BabyAI-%s-v0" % sc.level, sc.n, device=gpu, seeds=sc.seeds, auto_reset=sc.auto_reset, **kw)
    assert env.get_option("inplace") == int(ev["BBAI_INPLACE"]) and env.get_option("lookahead_period") == period
    if "BBAI_CONSUME_FUSED" in ev:
        assert env.get_option("consume_fused") == int(ev["BBAI_CONSUME_FUSED"])
    if "BBAI_PREGEN_LANE" in ev:
        assert env.get_option("pregen_lane") == int(ev["BBAI_PREGEN_LANE"])
    elif sc.level == G and ev["BBAI_INPLACE"] == "1":
        assert env.get_option("pregen_lane") == 1 and env.get_option("cplane") == 1
    assert env.get_option("reseed_levels") == 0
    if tokens:
        env.enable_instr_tokens()
    env.reset()
    return env


def _finish(env, want=None):
    assert env.get_option("gate_timeouts") == 0
    assert env.generator_failures() == 0
    assert env.get_option("reseed_levels") == 0          # (every reseed(levels=k) put the option back)
    if want is not None:
        assert env.reset_count() == want["starts"], (env.reset_count(), want["starts"])          # the parking move is counted like any reset
    env.close()


# ---- 1. the option -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_option_round_trip(gpu):
    from babyai_amd.engine import BatchedBabyAIEnv
    env = BatchedBabyAIEnv("BabyAI-GoToLocal-v0", 65, device=gpu, seeds=7)
    owned = env.get_option("owned")
    assert env.get_option("reseed_levels") == 0
    env.set_option("reseed_levels", 1)
    assert env.get_option("reseed_levels") == 1
    env.set_option("reseed_levels", 0)
    assert env.get_option("reseed_levels") == 0
    env.set_option("reseed_levels", -3)
    assert env.get_option("reseed_levels") == 0          # (stored as 0)
    env.set_option("reseed_levels", 1 << 20)
    assert env.get_option("reseed_levels") == 1 << 20    # (beyond any ring: the whole ring)
    assert env.get_option("owned") == owned              # no allocation, stream or event
    env.set_option("reseed_levels", 0)
    env.reset()
    _finish(env)


# ---- 2. bytes against the host model and the twin -------------------------------------------------------------------------------------------
def _both(gpu, monkeypatch, sc, want, ev, entry, tokens, profile=False, **kw):
    """The script on a handle with the script's depths and on its twin at depth 0; both held to the model."""
    import torch
    env, twin = _make(gpu, monkeypatch, sc, ev, tokens=tokens, **kw), _make(gpu, monkeypatch, sc, ev, tokens=tokens, **kw)
    for e in (env, twin):
        su._same("reset image", e.image.cpu().numpy(), want["reset"]["image"])
        if profile:
            e.profile(True)
    got = su.run_device(rl.WithLevels(env, sc.events), sc.events, entry)
    rl.assert_run(got, want)
    other = su.run_device(rl.WithLevels(twin, rl.twin_events(sc.events)), sc.events, entry)
    rl.assert_run(other, want, twin=True)
    unlisted = np.setdiff1d(np.arange(sc.n), sc.listed)
    for k, rows in got["steps"].items():                 # the unlisted envs: the twin's bytes at every step, whatever the model says
        for t, row in enumerate(rows):
            if row is not None:
                assert np.array_equal(su._bits(row)[unlisted], su._bits(other["steps"][k][t])[unlisted]), (k, t)
    parked = torch.as_tensor(want["parked"][-1], device=gpu)
    assert parked.any()
    if entry != "bot_rollout":                          # (bot_rollout's reward / done go to its history rows)
        assert (env.done[parked] == 1).all()
    if sc.auto_reset:
        act = env.bot_actions()
        assert (act[parked] == rl.A_DONE).all()          # the expert answers `done` for a parked env
    return env, twin, got


STEP = [("short", G, IP1), ("short", G, LANE0), ("short", G, IP0), ("short", BOSS, IP0), ("short", BOSS, IP0U), ("short", BOSS, IP1),
        ("frozen", G, IP1), ("frozen", G, IP0), ("frozen", BOSS, IP0)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,level,ev", STEP, ids=[_id(*c) for c in STEP])
def test_step(gpu, monkeypatch, name, level, ev):
    sc, want = rl.scenario(name, level, N), rl.model_run(name, level, N)
    env, twin, got = _both(gpu, monkeypatch, sc, want, ev, "step", True)
    assert len(got["steps"]["tokens"]) == want["T"]
    _finish(env, want)
    _finish(twin)


TICKS = [("short", G, IP1), ("short", G, LANE0), ("short", G, IP0F), ("short", BOSS, IP0), ("frozen", G, IP1), ("frozen", BOSS, IP0), ("frozen", G, IP0U)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,level,ev", TICKS, ids=[_id(*c) for c in TICKS])
def test_ticks(gpu, monkeypatch, name, level, ev):
    """rollout(step_tap=True) without a token buffer: k_step_ticks, several ticks per launch, the envs parking inside a launch."""
    sc, want = rl.scenario(name, level, N), rl.model_run(name, level, N)
    env, twin, got = _both(gpu, monkeypatch, sc, want, ev, "ticks" if sc.auto_reset else "ticks_frozen", False, profile=True)
    launches, ticks = env.profile_read()["k_step"][1], env.get_option("profile_step_ticks")
    assert ticks == want["T"] and launches < ticks, (launches, ticks)
    for e in (env, twin):
        e.profile(False)
    _finish(env, want)
    _finish(twin)


PIXELS = [("short", G, IP1), ("short", BOSS, IP0)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,level,ev", PIXELS, ids=[_id(*c) for c in PIXELS])
def test_pixel_steps(gpu, monkeypatch, name, level, ev):
    """Pixel steps (bbai_step_render, the step finding its dirty cells): the rendered picture of every env that is not parked is a full render of the
    model's image; a parked env's picture is a render of whatever its image row holds."""
    import torch
    sc, want = rl.scenario(name, level, N), rl.model_run(name, level, N)
    env = _make(gpu, monkeypatch, sc, ev, pixel=True, tile_size=8)
    env.set_option("render_delta_from_step", 1)
    scratch = torch.zeros_like(env.pixels)
    bad = []

    def after(kind, k):
        if kind == "step":
            scratch.zero_()
            same = (env.render_encoding(env.image, out=scratch) == env.pixels).reshape(N, -1).all(1)
            if not bool(same.all()):
                bad.append((k, same.logical_not().nonzero().reshape(-1)[:6].tolist()))

    got = su.run_device(rl.WithLevels(env, sc.events), sc.events, "dstore", after=after)
    rl.assert_run(got, want)
    assert not bad, "pixels differ from a full render of the image rows: %s" % bad[:4]
    _finish(env, want)


BOT = [(G, IP1), (G, IP0), (G, IP0U)]


@pytest.mark.gpu
@pytest.mark.parametrize("level,ev", BOT, ids=[_id(*c) for c in BOT])
def test_bot_rollout(gpu, monkeypatch, level, ev):
    sc, want = rl.scenario("bot", level, N), rl.model_run("bot", level, N)
    env, twin, got = _both(gpu, monkeypatch, sc, want, ev, "bot_rollout", True)
    before = want["parked_before"]
    assert before.any() and (got["bot"]["action"][before] == rl.A_DONE).all() and (got["bot"]["gave_up"][before] == 0).all()
    assert env.bot_stats() == want["bot_stats"]
    _finish(env, want)
    _finish(twin)


@pytest.mark.gpu
def test_done_action_mode(gpu, monkeypatch):
    sc, want = rl.scenario("short", G, N), rl.model_run("short", G, N, True)
    env, twin, _ = _both(gpu, monkeypatch, sc, want, IP1, "step", True, done_actions=True)
    assert env.lib.bbai_get_done_actions(env.handle) == 1
    _finish(env, want)
    _finish(twin)


@pytest.mark.gpu
def test_default_period(gpu, monkeypatch):
    """The default look-ahead (GoToLocal: period 64, 128 levels per ring + the live slot): every depth of the script is a short one there."""
    monkeypatch.delenv("BBAI_LOOKAHEAD")
    sc = rl.scenario("short", G, N)
    want = rl.ParkingModel(G, sc.seeds, ring=128).run(sc.events)
    assert want["parked"][-1].sum() > (rl.model_run("short", G, N)["parked"][-1]).sum()          # (depth 8 parks here)
    env = _make(gpu, monkeypatch, sc, IP1, tokens=True, period=64)
    got = su.run_device(rl.WithLevels(env, sc.events), sc.events, "step")
    rl.assert_run(got, want)
    _finish(env, want)


# ---- 3. checkpoint -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("level,ev", [(G, IP1), (G, IP0), (BOSS, IP0)], ids=["G-ip1", "G-ip0", "BOSS-ip0"])
def test_checkpoint_with_parked_and_half_spent_envs(gpu, monkeypatch, level, ev):
    import torch
    sc, want = rl.scenario("short", level, N), rl.model_run("short", level, N)
    cut = next(j for j, e in enumerate(sc.events) if e[0] == "steps" and sum(len(x[1]) for x in sc.events[:j + 1] if x[0] == "steps") == 26)
    head, tail = sc.events[:cut], sc.events[cut:]          # the head ends in front of steps 6 .. 25; cut it again at step 12
    steps = tail[0][1]
    head, tail = head + [("steps", steps[:6])], [("steps", steps[6:])] + tail[1:]
    at = 11
    assert want["parked"][at].any() and (~want["parked"][at][sc.listed]).sum() > 12          # parked, half-spent and whole-ring envs at the cut
    a = _make(gpu, monkeypatch, sc, ev, tokens=True)
    wa = rl.WithLevels(a, sc.events)
    su.run_device(wa, head, "step")
    blob = a.save_checkpoint()
    other = rl.Scenario(sc.name, sc.level, sc.n, sc.auto_reset, sc.events, sc.info, sc.seeds + np.uint64(999), sc.listed)
    d = _make(gpu, monkeypatch, other, ev, tokens=True)
    d.load_checkpoint(blob)
    for k in ("image", "direction", "reward", "reward64", "done"):          # (the current outputs are not part of the blob)
        getattr(d, k).copy_(getattr(a, k))
    wd = rl.WithLevels(d, sc.events)
    wd._depths.clear(); wd._depths.extend(wa._depths)
    ga, gd = su.run_device(wa, tail, "step"), su.run_device(wd, tail, "step")
    for k, rows in ga["steps"].items():
        for t, row in enumerate(rows):
            assert np.array_equal(su._bits(row), su._bits(gd["steps"][k][t])), (k, t)          # every byte, the parked envs' too
    for ca, cd in zip(ga["calls"], gd["calls"]):
        for k in ("image", "direction", "tokens"):
            assert np.array_equal(ca[k], cd[k]), k
    live = ~want["parked"][12:]
    for k in ("image", "done", "reward64"):
        assert np.array_equal(su._bits(np.stack(gd["steps"][k]))[live], su._bits(want["steps"][k][12:])[live]), k
    assert a.reset_count() == d.reset_count() == want["starts"]
    _finish(a)
    _finish(d)


# ---- 4. evaluate_policy ----------------------------------------------------------------------------------------------------------------
def _hash_policy():
    import torch
    weights = {}

    def policy(obs, t):
        img = obs["image"].reshape(obs["image"].shape[0], -1).to(torch.int64)
        if img.device not in weights:
            weights[img.device] = (torch.arange(img.shape[1], dtype=torch.int64, device=img.device) * 2654435761 + 12345) % 1000003
        h = (img * weights[img.device]).sum(1) + obs["direction"].to(torch.int64) * 7919
        return ((h >> 3) % 3).to(torch.uint8)
    return policy


@pytest.mark.gpu
@pytest.mark.parametrize("level,episodes,pool", [(G, 300, 64), ("GoToObjMaze", 24, 8)])
def test_pool_evaluation_with_one_level_per_reseed(gpu, monkeypatch, level, episodes, pool):
    from babyai_amd.engine import BatchedBabyAIEnv
    from babyai_amd.evaluate import evaluate_policy
    depths, real = [], BatchedBabyAIEnv.reseed

    def reseed(self, ids, seeds, levels=None):
        depths.append(levels)
        return real(self, ids, seeds, levels=levels)

    monkeypatch.setattr(BatchedBabyAIEnv, "reseed", reseed)
    name, policy = "BabyAI-%s-v0" % level, _hash_policy()
    want = evaluate_policy(policy, name, 10 ** 6, episodes, device=gpu)
    assert not depths
    pooled = evaluate_policy(policy, name, 10 ** 6, episodes, device=gpu, pool=pool, poll_every=4)
    assert depths and set(depths) == {None}
    del depths[:]
    got = evaluate_policy(policy, name, 10 ** 6, episodes, device=gpu, pool=pool, poll_every=4, reseed_levels=1)
    assert depths and set(depths) == {1}
    assert got == pooled == want
    if level == G:
        assert len(set(want["num_frames_per_episode"])) > 3 and any(r > 0 for r in want["return_per_episode"])          # (the seeds matter to the logs)


# ---- 5. collect_seeds ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("level,lo,count,pool", [(G, 1000, 512, 64), ("GoToObjMaze", 1000, 40, 8)])
def test_collect_seeds_with_one_level_per_reseed(gpu, monkeypatch, level, lo, count, pool):
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    from babyai_amd.imitation import DemoStore
    health, depths, real_close, real_reseed = [], [], BatchedBabyAIEnv.close, BatchedBabyAIEnv.reseed

    def close(self):
        if getattr(self, "handle", None):
            health.append((self.get_option("gate_timeouts"), self.generator_failures(), self.get_option("reseed_levels")))
        real_close(self)

    def reseed(self, ids, seeds, levels=None):
        depths.append(levels)
        return real_reseed(self, ids, seeds, levels=levels)

    monkeypatch.setattr(BatchedBabyAIEnv, "close", close)
    monkeypatch.setattr(BatchedBabyAIEnv, "reseed", reseed)
    name, seeds = "BabyAI-%s-v0" % level, list(range(lo, lo + count))
    store0, kept0 = DemoStore.collect_seeds(name, seeds, device=gpu, pool=pool)
    assert depths and set(depths) == {None}
    del depths[:]
    store1, kept1 = DemoStore.collect_seeds(name, seeds, device=gpu, pool=pool, reseed_levels=1)
    assert len(depths) > 1 and set(depths) == {1}
    assert np.array_equal(kept0, kept1) and len(kept1) > count // 2
    assert np.array_equal(store0.offset_host, store1.offset_host)
    for k in ("image", "direction", "action", "tokens", "offset"):
        assert torch.equal(getattr(store0, k), getattr(store1, k)), k
    assert health == [(0, 0, 0), (0, 0, 0)]
