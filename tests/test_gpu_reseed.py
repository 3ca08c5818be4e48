"""bbai_reseed (k_reseed_seed / k_reseed_consume, include/bbai.h; BatchedBabyAIEnv.reseed): env.seed(s); env.reset() for listed envs of a live
batch.  The listed envs behave as a fresh batch built with those seeds does -- first observation, mission, and every output of 200 steps across
many episodes and look-ahead windows --, no other env moves, the first observations are the CPU oracle's, the window edges and repeated calls
hold, every mode follows (frozen envs, done actions, token rows, the expert, pixels, checkpoints), the handle stays healthy, and
evaluate_policy's pool mode logs what the one-env-per-episode path logs.  BBAI_LOOKAHEAD=4 throughout: windows turn over every four ticks."""
import numpy as np
import pytest

N = 192
B = 4
KEYS = ("image", "direction", "reward", "reward64", "done")
RESET_ENV = 7


@pytest.fixture(autouse=True)
def _short_windows(monkeypatch):
    monkeypatch.setenv("BBAI_LOOKAHEAD", str(B))


def _setenv(monkeypatch, ev):
    for k, v in ev.items():
        monkeypatch.setenv(k, v)


def _make(level, n, gpu, seed, tokens=True, **kw):
    from babyai_amd.engine import BatchedBabyAIEnv
    env = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device=gpu, seeds=seed, **kw)
    if tokens:
        env.enable_instr_tokens()
    env.reset()
    return env


def _ids37(n, seed=3):
    """37 envs that include 0 and n - 1 and both sides of every 64-env boundary, in no order."""
    edge = [0, n - 1] + [b + d for b in range(64, n, 64) for d in (-1, 0) if 0 < b + d < n - 1]
    rng = np.random.RandomState(seed)
    rest = [i for i in rng.permutation(n) if i not in edge]
    ids = np.array(edge + rest[:37 - len(edge)], dtype=np.int64)
    assert len(ids) == 37 and len(set(ids.tolist())) == 37
    return rng.permutation(ids)


def _seeds(k, base=9000000):
    return np.arange(k, dtype=np.uint64) * np.uint64(17) + np.uint64(base)


def _acts(gpu, T, n, seed, resets=0.0):
    """Random actions; `resets`: the share of per-env reset commands among them (levels whose episodes outlast the test end some that way)."""
    import torch
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 7, size=(T, n)).astype(np.uint8)
    if resets:
        a[rng.rand(T, n) < resets] = RESET_ENV
    return torch.as_tensor(a, device=gpu)


def _run(env, acts, extra=("instr",)):
    """Step through acts[T, n] without a host synchronisation; every output of every step, stacked on the device."""
    import torch
    out = {k: [] for k in KEYS + tuple(extra)}
    for t in range(acts.shape[0]):
        env.step(acts[t])
        for k in KEYS + tuple(extra):
            out[k].append(getattr(env, k).clone())
    return {k: torch.stack(v) for k, v in out.items()}


def _assert_same(a, b, cols_a=None, cols_b=None, keys=KEYS + ("instr",), what=""):
    import torch
    for k in keys:
        x = a[k] if cols_a is None else a[k][:, cols_a]
        y = b[k] if cols_b is None else b[k][:, cols_b]
        if x.dtype == torch.float64:
            x, y = x.view(torch.int64), y.view(torch.int64)          # the bit pattern
        if not torch.equal(x, y):
            bad = (x != y).reshape(x.shape[0], x.shape[1], -1).any(-1).nonzero()[:6].tolist()
            raise AssertionError("%s %s differs at (step, column) %s" % (what, k, bad))


def _healthy(*envs):
    for e in envs:
        assert e.get_option("gate_timeouts") == 0
        e.close()


def _dev(gpu, a):
    import torch
    return torch.as_tensor(np.asarray(a, dtype=np.int64), device=gpu)


def _listed_vs_fresh(gpu, level, n, pre, steps, resets=0.0, kw=None, ids=None, new_seeds=None, a=None, c=None, base=1234):
    """Handle `a` (n envs, `pre` random steps behind its reset; built here unless given, with its twin `c`), reseeded at `ids`, against a fresh batch
    of those seeds and -- the unlisted envs -- against the twin that was not reseeded.  Returns (a, b, c) for further checks."""
    import torch
    kw = kw or {}
    if a is None:
        a, c = _make(level, n, gpu, base, **kw), _make(level, n, gpu, base, **kw)
        p = _acts(gpu, pre, n, 1, resets)
        _run(a, p); _run(c, p)
    ids = _ids37(n) if ids is None else ids
    new_seeds = _seeds(len(ids)) if new_seeds is None else new_seeds
    valid = (ids >= 0) & (ids < n)
    tids = _dev(gpu, ids[valid])
    unl = _dev(gpu, np.setdiff1d(np.arange(n), ids[valid]))
    resets0, fails0 = a.reset_count(), a.generator_failures()
    obs = a.reseed(ids, new_seeds)
    b = _make(level, int(valid.sum()), gpu, new_seeds[valid], **kw)
    assert obs["image"] is a.image
    assert torch.equal(a.image[tids], b.image) and torch.equal(a.direction[tids], b.direction), "first observation"
    assert torch.equal(a.instr[tids], b.instr)
    ma, mb = a.missions(), b.missions()
    assert [ma[int(i)] for i in ids[valid]] == mb
    assert a.reset_count() - resets0 == int(valid.sum())
    assert a.generator_failures() == fails0 == c.generator_failures()
    for k in ("image", "direction", "instr"):
        assert torch.equal(getattr(a, k)[unl], getattr(c, k)[unl]), k
    ab = _acts(gpu, steps, len(tids), 2, resets)
    aa = _acts(gpu, steps, n, 3, resets)
    aa[:, tids] = ab
    oa, ob, oc = _run(a, aa), _run(b, ab), _run(c, aa)
    _assert_same(oa, ob, cols_a=tids, what="listed env vs fresh batch:")
    _assert_same(oa, oc, cols_a=unl, cols_b=unl, what="unlisted env vs twin:")
    return a, b, c, ob


# ---- 1 + 2. listed envs equal a fresh batch; nothing else moves -----------------------------------------------------------------------------
MAIN = [(lv, {"BBAI_INPLACE": ip}, N) for lv in ("GoToLocal", "BossLevel", "PutNextS5N2Carrying") for ip in ("0", "1")] + [
    ("GoToLocal", {"BBAI_INPLACE": "1", "BBAI_PREGEN_LANE": "0"}, N), ("GoToLocal", {"BBAI_INPLACE": "0", "BBAI_PREGEN_LANE": "0"}, N),
    ("GoToLocal", {"BBAI_INPLACE": "1", "BBAI_CPLANE": "0"}, N), ("GoToLocal", {"BBAI_INPLACE": "0", "BBAI_VPLANE": "0"}, N),
    ("GoToLocal", {"BBAI_INPLACE": "0", "BBAI_CONSUME_FUSED": "0"}, N), ("GoToLocal", {"BBAI_INPLACE": "0", "BBAI_CONSUME_FUSED": "1"}, N),
    ("GoToLocal", {"BBAI_INPLACE": "1", "BBAI_LOOKAHEAD_STREAMS": "2"}, N), ("BossLevel", {"BBAI_INPLACE": "0", "BBAI_LOOKAHEAD_STREAMS": "2"}, N),
    ("GoToLocal", {"BBAI_INPLACE": "1"}, 65), ("GoToLocal", {"BBAI_INPLACE": "0"}, 65)]
MAIN_IDS = ["%s-%s-n%d" % (lv, "-".join("%s%s" % (k[5:].lower(), v) for k, v in sorted(ev.items())), n) for lv, ev, n in MAIN]


@pytest.mark.gpu
@pytest.mark.parametrize("level,ev,n", MAIN, ids=MAIN_IDS)
def test_listed_envs_equal_a_fresh_batch_and_nothing_else_moves(gpu, monkeypatch, level, ev, n):
    """22 steps behind the reset the call lands inside a window; 200 steps behind it every GoToLocal env starts three episodes at least (64 steps
    at most each), and the maze and the start-carry level end theirs by reset commands in the action stream."""
    _setenv(monkeypatch, ev)
    resets = 0.0 if level == "GoToLocal" else 0.08
    a, b, c, ob = _listed_vs_fresh(gpu, level, n, 22, 200, resets)
    for opt, var in (("inplace", "BBAI_INPLACE"), ("pregen_lane", "BBAI_PREGEN_LANE"), ("consume_fused", "BBAI_CONSUME_FUSED"), ("lookahead_streams", "BBAI_LOOKAHEAD_STREAMS")):
        if var in ev:
            assert a.get_option(opt) == int(ev[var]), opt
    assert a.get_option("lookahead_period") == B
    assert int((ob["done"] != 0).sum(0).min()) >= 3          # every listed env went through several episodes of its new stream
    _healthy(a, b, c)


# ---- 3. against the CPU oracle --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("level", ["GoToLocal", "BossLevel"])
def test_first_observation_and_mission_are_the_oracles(gpu, level):
    from test_gpu_parity import _oracle_envs
    env = _make(level, N, gpu, 77)
    _run(env, _acts(gpu, 22, N, 4))
    ids, new_seeds = _ids37(N, seed=5), _seeds(37, base=31337)
    obs = env.reseed(ids, new_seeds)
    image, direction, missions = obs["image"].cpu().numpy(), obs["direction"].cpu().numpy(), obs["mission"]
    for k, ref in enumerate(_oracle_envs(level, new_seeds)):
        want = ref.reset()
        i = int(ids[k])
        assert np.array_equal(image[i], want["image"]) and int(direction[i]) == want["direction"], (k, i)
        assert missions[i] == want["mission"], (k, i)
    _healthy(env)


# ---- 4. window edges and repeats --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("inplace", ["0", "1"])
@pytest.mark.parametrize("pre,between", [(B - 1, 2), (2 * B - 2, 0), (B + 1, 1)], ids=["position0", "positionB-1", "middle"])
def test_window_edges_and_the_same_env_twice_in_one_window(gpu, monkeypatch, inplace, pre, between):
    """reset() is consume-tick 0 and every auto-resetting step one more: `pre` steps put the call in front of tick pre + 1.  The listed envs are
    reseeded, stepped `between` times (the window does not turn over) and reseeded again: the second call's seeds are what counts."""
    monkeypatch.setenv("BBAI_INPLACE", inplace)
    a, c = _make("GoToLocal", N, gpu, 555), _make("GoToLocal", N, gpu, 555)
    p = _acts(gpu, pre + between, N, 6)
    _run(a, p[:pre]); _run(c, p)
    assert (pre + 1) % B == {B - 1: 0, 2 * B - 2: B - 1, B + 1: 2}[pre] and (pre + 1) % B + between < B
    ids = _ids37(N, seed=7)
    a.reseed(ids, _seeds(37, base=111))
    if between:
        _run(a, p[pre:])
    a, b, c, _ = _listed_vs_fresh(gpu, "GoToLocal", N, 0, 40, ids=ids, new_seeds=_seeds(37, base=222), a=a, c=c)
    _healthy(a, b, c)


@pytest.mark.gpu
@pytest.mark.parametrize("level,inplace", [("GoToLocal", "0"), ("GoToLocal", "1"), ("BossLevel", "0")])
def test_every_env_listed_is_a_fresh_handles_seed_and_reset(gpu, monkeypatch, level, inplace):
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv, EngineError
    monkeypatch.setenv("BBAI_INPLACE", inplace)
    new_seeds = _seeds(N, base=4242)
    a = _make(level, N, gpu, 50)
    _run(a, _acts(gpu, 22, N, 8))
    resets0 = a.reset_count()
    obs = a.reseed(None, new_seeds)
    assert a.reset_count() - resets0 == N
    # ... and a handle that was seeded but never reset takes every env, and nothing less
    u = BatchedBabyAIEnv("BabyAI-%s-v0" % level, N, device=gpu, seeds=50)
    u.enable_instr_tokens()
    with pytest.raises(EngineError):
        u.reseed([1, 2], [5, 6])
    u.reseed(None, new_seeds)
    f = _make(level, N, gpu, new_seeds)
    for h in (a, u):
        assert torch.equal(h.image, f.image) and torch.equal(h.direction, f.direction) and torch.equal(h.instr, f.instr)
    assert obs["mission"][:] == f.missions()
    acts = _acts(gpu, 40, N, 9, 0.0 if level == "GoToLocal" else 0.05)
    oa, ou, of = _run(a, acts), _run(u, acts), _run(f, acts)
    _assert_same(oa, of, what="every env reseeded vs fresh handle:")
    _assert_same(ou, of, what="never-reset handle reseeded vs fresh handle:")
    _healthy(a, u, f)


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", ["0", "1"])
def test_padded_id_lists_and_empty_calls(gpu, monkeypatch, inplace):
    import torch
    monkeypatch.setenv("BBAI_INPLACE", inplace)
    a, c = _make("GoToLocal", N, gpu, 60), _make("GoToLocal", N, gpu, 60)
    p = _acts(gpu, 22, N, 10)
    _run(a, p); _run(c, p)
    resets0 = a.reset_count()
    image0 = a.image.clone()
    for ids, seeds in (([], []), (torch.zeros((0,), dtype=torch.int64, device=gpu), torch.zeros((0,), dtype=torch.int64, device=gpu)),
                       (torch.full((6,), -1, dtype=torch.int64, device=gpu), torch.arange(6, dtype=torch.int64, device=gpu)),
                       (torch.full((3,), N, dtype=torch.int64, device=gpu), torch.arange(3, dtype=torch.int64, device=gpu))):
        obs = a.reseed(ids, seeds)
        assert torch.equal(obs["image"], image0)
    assert a.reset_count() == resets0
    ids = _ids37(N, seed=11)
    padded = np.full(37 + 16, -1, dtype=np.int64)
    padded[np.arange(37) + np.arange(37) * 16 // 37] = ids          # the padding scattered through the list
    pad = padded.copy()
    pad[np.flatnonzero(padded == -1)[::2]] = N                       # -1 and N alternate
    assert (pad == -1).sum() == 8 and (pad == N).sum() == 8 and np.array_equal(pad[(pad >= 0) & (pad < N)], ids)
    a, b, c, _ = _listed_vs_fresh(gpu, "GoToLocal", N, 0, 40, ids=pad, new_seeds=_seeds(len(pad), base=333), a=a, c=c)
    _healthy(a, b, c)


# ---- 5. modes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("inplace", ["0", "1"])
def test_frozen_listed_envs_are_live_again_and_the_others_stay_frozen(gpu, monkeypatch, inplace):
    import torch
    monkeypatch.setenv("BBAI_INPLACE", inplace)
    kw = dict(auto_reset=False)
    a, c = _make("GoToLocal", N, gpu, 70, **kw), _make("GoToLocal", N, gpu, 70, **kw)
    p = _acts(gpu, 70, N, 12)                     # 64 steps end every GoToLocal episode: the whole batch is frozen
    _run(a, p); _run(c, p)
    assert bool((a.done != 0).all())
    a, b, c, ob = _listed_vs_fresh(gpu, "GoToLocal", N, 0, 40, kw=kw, a=a, c=c)
    tids = _dev(gpu, _ids37(N))
    unl = _dev(gpu, np.setdiff1d(np.arange(N), _ids37(N)))
    assert bool((a.done[unl] != 0).all()) and not bool((ob["done"][0] != 0).all())
    assert not bool((a.done[tids] != 0).all())          # (40 steps: some of the new episodes are still running)
    _healthy(a, b, c)


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", ["0", "1"])
def test_done_action_mode_starts_with_a_cleared_last_step_match(gpu, monkeypatch, inplace):
    """GoToLocal under done actions: the listed envs include those that stand in front of their target (lastStepMatch set) at the call; behind it
    their byte is clear, and `done` as the first action fails in the listed envs as it does in the fresh batch."""
    import torch
    monkeypatch.setenv("BBAI_INPLACE", inplace)
    kw = dict(done_actions=True)
    a, c = _make("GoToLocal", N, gpu, 77, **kw), _make("GoToLocal", N, gpu, 77, **kw)
    pre = _acts(gpu, 45, N, 4) % 6
    matched = None
    for t in range(45):
        a.step(pre[t]); c.step(pre[t])
        if t >= 21:
            snap = a.save_state()
            matched = (snap.lsm != 0) & (snap.hot[:, 13] == 0)
            if bool(matched.any()):
                break
    assert bool(matched.any()), "no env stood in front of its target in 45 steps: choose other seeds"
    m = matched.nonzero().reshape(-1).cpu().numpy()
    rest = np.array([i for i in _ids37(N, seed=13) if i not in set(m.tolist())], dtype=np.int64)
    ids = np.concatenate([m, rest])[:37]
    new_seeds = _seeds(37, base=808)
    tids = _dev(gpu, ids)
    a.reseed(ids, new_seeds)
    assert not bool(a.save_state(ids).lsm.any())
    b = _make("GoToLocal", 37, gpu, new_seeds, **kw)
    assert torch.equal(a.image[tids], b.image)
    ab = _acts(gpu, 40, 37, 14) % 6
    ab[0] = 6                                    # `done` right away: no env of a fresh batch has matched yet
    ab[9] = 6
    aa = _acts(gpu, 40, N, 15) % 6
    aa[:, tids] = ab
    unl = _dev(gpu, np.setdiff1d(np.arange(N), ids))
    oa, ob, oc = _run(a, aa), _run(b, ab), _run(c, aa)
    assert bool((oa["reward64"][0][tids] == 0).all())
    _assert_same(oa, ob, cols_a=tids, what="done-action mode, listed vs fresh:")
    _assert_same(oa, oc, cols_a=unl, cols_b=unl, what="done-action mode, unlisted vs twin:")
    _healthy(a, b, c)


@pytest.mark.gpu
@pytest.mark.parametrize("level,inplace", [("GoToLocal", "0"), ("GoToLocal", "1"), ("BossLevel", "0")])
def test_token_rows_and_a_fresh_expert(gpu, monkeypatch, level, inplace):
    import torch
    monkeypatch.setenv("BBAI_INPLACE", inplace)
    a = _make(level, N, gpu, 100)
    prev = None
    for t in range(10):              # the expert on every env: its plans expect step 10 next
        act = a.bot_actions(prev).clone()
        act[act == a.BOT_GAVE_UP] = 6
        a.step(act)
        prev = act
    before = a.instr.clone()
    ids, new_seeds = _ids37(N, seed=22), _seeds(37, base=606)
    tids = _dev(gpu, ids)
    unl = _dev(gpu, np.setdiff1d(np.arange(N), ids))
    a.reseed(ids, new_seeds)
    b = _make(level, 37, gpu, new_seeds)
    assert torch.equal(a.instr[tids], b.instr)
    assert torch.equal(a.instr[unl], before[unl])
    assert not torch.equal(a.instr[tids], before[tids])
    for t in range(3):
        got, want = a.bot_actions(prev if t else None).clone(), b.bot_actions(None if t == 0 else wprev).clone()
        assert torch.equal(got[tids], want), ("expert decision", t)
        got[got == a.BOT_GAVE_UP] = 6
        want[want == b.BOT_GAVE_UP] = 6
        a.step(got); b.step(want)
        prev, wprev = got, want
        assert torch.equal(a.image[tids], b.image)
    _healthy(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("tile_size", [8, 16])
def test_pixels_follow_a_reseed(gpu, tile_size):
    import torch
    env = _make("GoToLocal", N, gpu, 800, tokens=False, pixel=True, tile_size=tile_size)
    acts = _acts(gpu, 25, N, 19)
    for t in range(22):
        env.step(acts[t])
    obs = env.reseed(_ids37(N, seed=20), _seeds(37, base=909))
    assert obs["image"] is env.pixels
    assert torch.equal(obs["image"], env.render_encoding(env.image, out=torch.zeros_like(env.pixels))), "after reseed"
    for t in range(22, 25):
        obs, _, _, _ = env.step(acts[t])
        assert torch.equal(obs["image"], env.render_encoding(env.image, out=torch.zeros_like(env.pixels))), ("step", t)
    _healthy(env)


@pytest.mark.gpu
@pytest.mark.parametrize("level,inplace", [("GoToLocal", "1"), ("GoToLocal", "0"), ("BossLevel", "0")])
def test_a_checkpoint_right_after_a_reseed_continues_identically(gpu, monkeypatch, level, inplace):
    monkeypatch.setenv("BBAI_INPLACE", inplace)
    resets = 0.0 if level == "GoToLocal" else 0.05
    a = _make(level, N, gpu, 300)
    _run(a, _acts(gpu, 22, N, 30, resets))
    a.reseed(_ids37(N, seed=31), _seeds(37, base=707))
    blob = a.save_checkpoint()
    d = _make(level, N, gpu, 1)
    d.load_checkpoint(blob)
    acts = _acts(gpu, 60, N, 32, resets)
    oa, od = _run(a, acts), _run(d, acts)
    _assert_same(oa, od, what="checkpoint behind a reseed:")
    _healthy(a, d)


# ---- 6. evaluate_policy(pool=...) ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pool_evaluation_logs_what_the_default_path_logs(gpu):
    import torch
    from babyai_amd.evaluate import evaluate_policy
    weights = {}
    seen = {"starts": 0, "keys": set()}

    def policy(obs, t):
        """a fixed hash of the image bytes and the direction, mapped to an action: left, right or forward (an action that leaves the observation as
        it is would be chosen again for ever: the episode would only time out, whatever its seed)"""
        img = obs["image"].reshape(obs["image"].shape[0], -1).to(torch.int64)
        if img.device not in weights:
            weights[img.device] = (torch.arange(img.shape[1], dtype=torch.int64, device=img.device) * 2654435761 + 12345) % 1000003
        h = (img * weights[img.device]).sum(1) + obs["direction"].to(torch.int64) * 7919
        seen["keys"] |= set(obs.keys())
        if "episode_start" in obs:
            assert obs["episode_start"].dtype == torch.uint8 and obs["episode_start"].shape == (img.shape[0],)
            seen["starts"] += int(obs["episode_start"].sum())
        return ((h >> 3) % 3).to(torch.uint8)

    want = evaluate_policy(policy, "BabyAI-GoToLocal-v0", 10 ** 6, 300, device=gpu)
    assert "episode_start" not in seen["keys"]
    got = evaluate_policy(policy, "BabyAI-GoToLocal-v0", 10 ** 6, 300, device=gpu, pool=64, poll_every=4)
    assert seen["starts"] == 300
    for k in ("seed_per_episode", "num_frames_per_episode", "return_per_episode"):
        assert got[k] == want[k], k
    print("frames", sorted(set(want["num_frames_per_episode"])), "successes", sum(r > 0 for r in want["return_per_episode"]))
    assert len(set(want["num_frames_per_episode"])) > 3 and any(r > 0 for r in want["return_per_episode"])          # (the seeds matter to the logs)
