"""bbai_reseed and bbai_load_state under EVERY step entry, against the host build.  tests/test_gpu_reseed.py and tests/test_gpu_state_snapshot.py
check the calls themselves, with env.step() behind them and another engine handle as the reference; here the scripted runs of
tests/scenario_util.py (reseeds at window positions 0, 1 and B - 1, an env that consumes B + 1 slots in one window, saves, loads with one row in
three envs, a state loaded one step from its time limit, both calls mixed inside one window, envs reseeded in consecutive windows while they finish on
every tick, every env reseeded at once, frozen envs reseeded and loaded, a reset() of the whole batch behind that) go through

    step             env.step, token rows registered                             k_step, k_tokens by `dones`
    ticks            rollout(step_tap=True), every env tapped, no token buffer   k_step_ticks: several ticks per launch, the tap rows by the stepping lanes
    ticks_frozen     the same with auto_reset=False                              k_step_ticks, not capped by the window
    rollout_tokens   rollout with an id tap, token rows registered               one k_step + k_tokens + k_tap per tick
    step_tapped      step_tapped, listed and unlisted envs tapped                k_step with tap rows
    dstore           pixel steps, render_delta_from_step = 1                     step_dirty + k_render_dstore at both piece sizes
    dstore_split     ... with step_render_split = 1                              the batch in two halves
    dstore_abi       ... the calls through the C ABI, no render behind them      the shadow is a frame older than the state
    bot_rollout      bot_rollout chunks between the events                       k_bot (dead_action = RESET_ENV), gave_up rows, token rows per step

and EVERY byte of every step's outputs, of every post-call observation and of every snapshot row, of all n envs, equals the host model's
(ScenarioModel on hostsim_util.HostBatch; pinned without a GPU by tests/test_scenario_host.py): exact equality, rewards by bit pattern.  Every case
ends with gate_timeouts == 0, generator_failures() == 0 and reset_count() equal to the model's count of episode starts, and asserts that the path
it is named after ran.  BBAI_LOOKAHEAD=4 throughout."""
import numpy as np
import pytest

import scenario_util as su

B = su.B
G, BOSS, PUT = "GoToLocal", "BossLevel", "PutNextS5N2Carrying"
IP0, IP1 = {"BBAI_INPLACE": "0"}, {"BBAI_INPLACE": "1"}
# a single room in the classic layout consumes unfused by default (k_consume behind the step): the entries that need the step to leave the final
# outputs behind (several ticks per launch, the step's dirty cells) get the fused consume there
IP0F = {"BBAI_INPLACE": "0", "BBAI_CONSUME_FUSED": "1"}
IP0U = {"BBAI_INPLACE": "0", "BBAI_CONSUME_FUSED": "0"}


@pytest.fixture(autouse=True)
def _short_windows(monkeypatch):
    monkeypatch.setenv("BBAI_LOOKAHEAD", str(B))


def _id(*parts):
    out = []
    for p in parts:
        out.append("-".join("%s%s" % (k[5:].lower(), v) for k, v in sorted(p.items())) if isinstance(p, dict) else str(p))
    return "-".join(out)


def _make(gpu, monkeypatch, sc, ev, tokens=False, **kw):
    from babyai_amd.engine import BatchedBabyAIEnv
    for k, v in ev.items():
        monkeypatch.setenv(k, v)
    env = BatchedBabyAIEnv("BabyAI-%s-v0" % sc.level, sc.n, device=gpu, seeds=sc.seeds, auto_reset=sc.auto_reset, **kw)
    assert env.get_option("inplace") == int(ev["BBAI_INPLACE"]) and env.get_option("lookahead_period") == B
    if "BBAI_CONSUME_FUSED" in ev:
        assert env.get_option("consume_fused") == int(ev["BBAI_CONSUME_FUSED"])
    if tokens:
        env.enable_instr_tokens()
    env.reset()
    return env


def _finish(env, model):
    """What every case ends with."""
    assert env.get_option("gate_timeouts") == 0
    assert env.generator_failures() == 0
    assert env.reset_count() == model["starts"], (env.reset_count(), model["starts"])
    env.close()


def _check_reset(env, model, tokens):
    su._same("reset image", env.image.cpu().numpy(), model["reset"]["image"])
    su._same("reset direction", env.direction.cpu().numpy(), model["reset"]["direction"])
    if tokens:
        su._same("reset tokens", env.instr.cpu().numpy(), model["reset"]["tokens"])


# ---- step ------------------------------------------------------------------------------------------------------------------------------
STEP = [("main", G, 192, IP0), ("main", G, 192, IP1), ("main", BOSS, 192, IP0), ("main", BOSS, 192, IP1), ("main", PUT, 192, IP0), ("main", PUT, 192, IP1),
        ("main", G, 192, IP0U), ("main", G, 65, IP0), ("main", G, 65, IP1), ("mixed", G, 192, IP0), ("mixed", G, 192, IP1), ("mixed", BOSS, 192, IP0),
        ("storm", G, 192, IP0), ("storm", G, 192, IP1), ("storm", BOSS, 192, IP0)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,level,n,ev", STEP, ids=[_id(*c) for c in STEP])
def test_step(gpu, monkeypatch, name, level, n, ev):
    sc, model = su.scenario(name, level, n), su.model_run(name, level, n)
    env = _make(gpu, monkeypatch, sc, ev, tokens=True)
    _check_reset(env, model, True)
    got = su.run_device(env, sc.events, "step")
    su.assert_equals_model(got, model)
    assert len(got["steps"]["tokens"]) == model["T"]
    _finish(env, model)


# ---- ticks, ticks_frozen ------------------------------------------------------------------------------------------------------------------
TICKS = [("main", G, 192, IP0F), ("main", G, 192, IP1), ("main", BOSS, 192, IP0), ("main", BOSS, 192, IP1), ("main", PUT, 192, IP1), ("main", G, 65, IP0F),
         ("main", G, 65, IP1), ("main", PUT, 192, IP0F), ("mixed", G, 192, IP0F), ("mixed", G, 192, IP1), ("mixed", BOSS, 192, IP0),
         ("storm", G, 192, IP0F), ("storm", G, 192, IP1), ("storm", BOSS, 192, IP0), ("storm", BOSS, 192, IP1),
         ("frozen", G, 192, IP0), ("frozen", G, 192, IP1), ("frozen", BOSS, 192, IP0), ("frozen", G, 65, IP1), ("frozen", G, 192, IP0U)]


def _ticks(gpu, monkeypatch, name, level, n, ev, side=False):
    import torch
    sc, model = su.scenario(name, level, n), su.model_run(name, level, n)
    entry = "ticks" if sc.auto_reset else "ticks_frozen"
    env = _make(gpu, monkeypatch, sc, ev)
    assert getattr(env, "instr", None) is None          # (a registered token buffer keeps one step per launch)
    _check_reset(env, model, False)
    env.profile(True)
    if side:
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(device=gpu)
        with torch.cuda.stream(stream):          # the calls and the rollouts behind them on this stream, nothing but stream order between them
            got = su.run_device(env, sc.events, entry)
    else:
        got = su.run_device(env, sc.events, entry)
    launches, ticks = env.profile_read()["k_step"][1], env.get_option("profile_step_ticks")
    env.profile(False)
    su.assert_equals_model(got, model)
    assert ticks == model["T"], (ticks, model["T"])
    assert launches < ticks, "%d k_step launches for %d steps: the multi-tick path did not run" % (launches, ticks)
    if not sc.auto_reset:          # one launch per rollout call, however many windows' worth of ticks it takes
        chunks = [len(e[1]) for e in sc.events if e[0] == "steps"]
        assert launches == len(chunks) and max(chunks) > B
    assert any(e.get("all") for e in model["log"]) == (name == "storm")
    _finish(env, model)


@pytest.mark.gpu
@pytest.mark.parametrize("name,level,n,ev", TICKS, ids=[_id(*c) for c in TICKS])
def test_ticks(gpu, monkeypatch, name, level, n, ev):
    _ticks(gpu, monkeypatch, name, level, n, ev)


@pytest.mark.gpu
def test_ticks_with_the_calls_on_another_stream(gpu, monkeypatch):
    """As test_gpu_state_snapshot's test_a_call_on_another_stream_is_ordered_with_the_step_behind_it: the mixed scenario's reseeds, saves and loads on
    a stream that is not the default one, the multi-tick rollouts behind them with no synchronisation in between."""
    _ticks(gpu, monkeypatch, "mixed", G, 192, IP1, side=True)


# ---- rollout_tokens -------------------------------------------------------------------------------------------------------------------
ROLL = [("main", G, 192, IP0), ("main", G, 192, IP1), ("main", BOSS, 192, IP0), ("main", G, 192, IP0U), ("main", G, 65, IP1), ("storm", G, 192, IP1)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,level,n,ev", ROLL, ids=[_id(*c) for c in ROLL])
def test_rollout_tokens(gpu, monkeypatch, name, level, n, ev):
    sc, model = su.scenario(name, level, n), su.model_run(name, level, n)
    env = _make(gpu, monkeypatch, sc, ev, tokens=True)
    env.profile(True)
    got = su.run_device(env, sc.events, "rollout_tokens")
    launches, ticks = env.profile_read()["k_step"][1], env.get_option("profile_step_ticks")
    env.profile(False)
    su.assert_equals_model(got, model)
    assert sum(r is not None for r in got["steps"]["tokens"]) == sum(e[0] == "steps" for e in sc.events)
    assert launches == ticks == model["T"], (launches, ticks)
    _finish(env, model)


# ---- step_tapped ---------------------------------------------------------------------------------------------------------------------
TAPPED = [("main", G, 192, IP0), ("main", G, 192, IP1), ("main", BOSS, 192, IP0), ("main", G, 192, IP0U), ("main", G, 65, IP1), ("main", PUT, 192, IP0), ("frozen", G, 192, IP1), ("frozen", G, 192, IP0)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,level,n,ev", TAPPED, ids=[_id(*c) for c in TAPPED])
def test_step_tapped(gpu, monkeypatch, name, level, n, ev):
    sc, model = su.scenario(name, level, n), su.model_run(name, level, n)
    listed = sorted({int(i) for e in model["log"] for i in e["ids"]})
    rng = np.random.RandomState(4)
    unlisted = np.setdiff1d(np.arange(n), listed)
    tap_ids = rng.permutation(np.concatenate([rng.choice(listed, len(listed) // 2, replace=False), rng.choice(unlisted, 9, replace=False)]))
    env = _make(gpu, monkeypatch, sc, ev)
    got = su.run_device(env, sc.events, "step_tapped", tap_ids=tap_ids)
    su.assert_equals_model(got, model, tap_ids=tap_ids)
    assert len(got["tapped"]["done"]) == model["T"]
    _finish(env, model)


# ---- dstore, dstore_split, dstore_abi ------------------------------------------------------------------------------------------------------
DSTORE = [("dstore", "main", G, 192, IP1, 64), ("dstore", "main", G, 192, IP1, 128), ("dstore", "main", G, 192, IP0F, 64), ("dstore", "main", G, 192, IP0F, 128),
          ("dstore", "main", BOSS, 192, IP0, 64), ("dstore", "main", BOSS, 192, IP0, 128), ("dstore", "main", G, 65, IP1, 128),
          ("dstore", "main", PUT, 192, IP1, 64), ("dstore", "mixed", G, 192, IP1, 64), ("dstore", "mixed", G, 192, IP1, 128), ("dstore", "mixed", BOSS, 192, IP0, 64),
          ("dstore", "storm", G, 192, IP1, 128), ("dstore", "storm", BOSS, 192, IP0, 64),
          ("dstore_split", "main", G, 192, IP1, 64), ("dstore_split", "main", G, 192, IP1, 128), ("dstore_split", "main", G, 192, IP0F, 128),
          ("dstore_split", "main", BOSS, 192, IP0, 64), ("dstore_split", "main", G, 65, IP1, 128), ("dstore_split", "storm", G, 192, IP1, 64),
          ("dstore_abi", "main", G, 192, IP1, 64), ("dstore_abi", "main", G, 192, IP1, 128), ("dstore_abi", "main", G, 192, IP0F, 64),
          ("dstore_abi", "main", BOSS, 192, IP0, 128), ("dstore_abi", "main", G, 65, IP1, 64), ("dstore_abi", "storm", G, 192, IP0F, 128)]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,name,level,n,ev,piece", DSTORE, ids=[_id(*c) for c in DSTORE])
def test_dstore(gpu, monkeypatch, entry, name, level, n, ev, piece):
    """The step finds the dirty cells against the shadow (step_dirty), the render only stores them (k_render_dstore): after a reseed or a load the
    shadow is compared with a frame that changed wholesale -- through the call's own delta render, or (dstore_abi: no render between the call and
    the next bbai_step_render, which include/bbai.h allows) while it still describes the frame before the call."""
    import torch
    sc, model = su.scenario(name, level, n), su.model_run(name, level, n)
    env = _make(gpu, monkeypatch, sc, ev, pixel=True, tile_size=8)
    env.set_option("render_delta_from_step", 1)
    env.set_option("render_piece_bytes", piece)
    if entry == "dstore_split":
        env.set_option("step_render_split", 1)
    assert env.get_option("render_delta_from_step") == 1 and env.get_option("render_piece_bytes") == piece and env.get_option("render_delta") == 1
    assert env.get_option("step_render_split") == (1 if entry == "dstore_split" else -1)
    want_steps = torch.as_tensor(model["steps"]["image"], device=gpu)
    want_calls = [torch.as_tensor(c["image"], device=gpu) for c in model["calls"]]
    scratch = torch.zeros_like(env.pixels)
    flags, where = [], []

    def pixels_are(image, what):
        """env.pixels against a full render of the MODEL's image into a zeroed buffer (a render into another buffer leaves the shadow alone)"""
        scratch.zero_()
        flags.append((env.render_encoding(image, out=scratch) == env.pixels).reshape(n, -1).all(1))
        where.append(what)

    def after(kind, k):
        if kind == "step":
            pixels_are(want_steps[k], "step %d" % k)
        elif entry != "dstore_abi":          # (the ABI calls leave the registered target alone: the next step's render brings it up to date)
            pixels_are(want_calls[k], "call %d" % k)

    pixels_are(torch.as_tensor(model["reset"]["image"], device=gpu), "reset")
    assert env.get_option("render_delta_valid") == 1
    got = su.run_device(env, sc.events, entry, after=after)
    assert env.get_option("render_delta_valid") == 1
    su.assert_equals_model(got, model)
    ok = torch.stack(flags).cpu().numpy()
    assert len(ok) == 1 + model["T"] + (0 if entry == "dstore_abi" else len(model["calls"]))
    bad = np.argwhere(~ok)
    assert not len(bad), "pixels differ from a full render of the host model's image: %s" % [(where[r], int(e)) for r, e in bad[:8]]
    _finish(env, model)


# ---- bot_rollout ---------------------------------------------------------------------------------------------------------------------
BOT = [(G, IP0), (G, IP1), (BOSS, IP0), (BOSS, IP1), (G, IP0U)]


@pytest.mark.gpu
@pytest.mark.parametrize("level,ev", BOT, ids=[_id(*c) for c in BOT])
def test_bot_rollout(gpu, monkeypatch, level, ev):
    """The expert's rollout between the events: a fresh Bot behind every reseed and load (and at every episode start), its decisions, the gave_up
    rows and the token rows of every step against HostBot's on the host model."""
    sc, model = su.scenario("bot", level, 65), su.model_run("bot", level, 65)
    env = _make(gpu, monkeypatch, sc, ev, tokens=True)
    _check_reset(env, model, True)
    got = su.run_device(env, sc.events, "bot_rollout")
    su.assert_equals_model(got, model)
    assert len(got["bot"]["action"]) == model["T"]
    su._same("final image", env.image.cpu().numpy(), model["steps"]["image"][-1])
    su._same("final direction", env.direction.cpu().numpy(), model["steps"]["direction"][-1])
    su._same("final tokens", env.instr.cpu().numpy(), model["steps"]["tokens"][-1])
    assert env.bot_stats() == model["bot_stats"], (env.bot_stats(), model["bot_stats"])
    _finish(env, model)
