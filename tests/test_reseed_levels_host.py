"""Short reseeds (include/bbai.h bbai_reseed, option "reseed_levels") without a GPU: the host model that parks (reseed_levels_util.ParkingModel)
pinned to the plain ScenarioModel wherever nothing is parked, and what each scripted run claims to reach, asserted on the model alone; the
`levels=` argument of BatchedBabyAIEnv.reseed on a bare env; and both pool schedulers -- evaluate._evaluate_pool and DemoStore.collect_seeds
-- on CPU tensors over the host build with `levels` honoured: their results with reseed_levels=1 equal the default's and the per-seed
episodes played one env at a time."""
import numpy as np
import pytest

import reseed_levels_util as rl
import scenario_util as su
import seed_demos_util as sd

B, RING = rl.B, rl.RING
N = 192
CASES = [("short", "GoToLocal"), ("short", "BossLevel"), ("frozen", "GoToLocal"), ("frozen", "BossLevel"), ("bot", "GoToLocal")]


# ---- the scenarios' own claims, on the model --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,level", CASES)
def test_listed_envs_cover_the_batch_edges_and_at_most_half_of_their_steps_are_parked(name, level):
    sc, want = rl.scenario(name, level, N), rl.model_run(name, level, N)
    assert len(sc.listed) == 37 and {0, N - 1, 63, 64, 127, 128} <= set(sc.listed.tolist())
    first, share = rl.parked_facts(want, sc)
    assert 0.0 < share <= 0.5, share
    assert not want["parked"][:, np.setdiff1d(np.arange(N), sc.listed)].any()          # no unlisted env ever parks
    assert want["parked"].shape == want["parked_before"].shape == (want["T"], N)
    assert (want["steps"]["done"][want["parked"]] == 1).all()                          # a parked env's done stays 1 ...
    p = want["parked"][1:] & want["parked"][:-1]
    if "again_at" in sc.info:          # (an env reseeded there may spend its one level in one step: parked on both sides of the call, another episode's reward)
        p[sc.info["again_at"] - 1] = False
    r = su._bits(want["steps"]["reward64"])
    assert (r[1:][p] == r[:-1][p]).all()                                               # ... and its reward the last episode's


@pytest.mark.parametrize("level", ["GoToLocal", "BossLevel"])
def test_short_scenario_parks_each_depth_where_it_says(level):
    sc, want = rl.scenario("short", level, N), rl.model_run("short", level, N)
    first, _ = rl.parked_facts(want, sc)
    g = sc.info["groups"]
    parked, done = want["parked"], want["steps"]["done"]
    for grp, k in zip(g, rl.DEPTHS):
        for part, s in zip(np.array_split(grp, 3), (3, 5, 6)):          # reseeded in front of window positions 0, 2 and 3
            assert (s + 1) % B == {3: 0, 5: 2, 6: 3}[s]
            for j, i in enumerate(part.tolist()):
                every = 1 if (j == 0 and s == 3) else 3
                ends = np.flatnonzero(done[s:25, i] != 0) + s          # the episode ends behind the reseed while the env is live
                if k < RING:
                    assert first[i] == ends[k - 1], (i, k, first[i])                 # the k-th end parks it, not one before ...
                    assert first[i] <= s + every * k - 1                             # ... the scripted one at the latest (random actions may end one earlier)
                else:
                    assert first[i] == -1                                            # the whole ring: never
    for i in sc.info["one_window"]:
        assert 3 <= first[i] <= 5                                                    # spent inside the window of steps 3 .. 6
    eight = int(g[3][0])
    assert int((done[3:11, eight] != 0).sum()) == 8 and first[eight] == -1           # depth RING: eight levels played, still live
    at = sc.info["again_at"]
    last = max(int(first[i]) for grp in g[:3] for i in grp)
    assert last + 2 * B <= at - 1 and parked[last:at, [i for grp in g[:3] for i in grp]].all()          # still parked two windows later
    assert parked[at - 1, sc.info["again1"]].all() and parked[at - 1, sc.info["again0"]].all()
    assert not parked[at, sc.info["again1"]].any() and not parked[at, sc.info["again0"]].any()          # back behind their reseeds
    a1, a0 = int(sc.info["again1"][0]), int(sc.info["again0"][0])
    assert parked[29:, a1].all()                                                     # depth 1 again: parks again, at step 29 at the latest
    assert not parked[26:, a0].any() and int((done[26:, a0] != 0).sum()) >= 3        # depth 0: three more episodes, never parked
    stay = [int(i) for i in g[0][5:]]
    assert parked[-1, stay].all()


def test_frozen_scenario_parks_by_the_reset_alone():
    sc, want = rl.scenario("frozen", "GoToLocal", N), rl.model_run("frozen", "GoToLocal", N)
    a, b, c = sc.info["groups"]
    at = sc.info["reset_at"]
    assert not want["parked"][:at].any()                                             # frozen at the end of each level as ever, not parked
    assert (want["steps"]["done"][at - 1] == 1).all()
    assert want["parked"][at:, a].all() and not want["parked"][:, b].any() and not want["parked"][:, c].any()
    assert want["parked_calls"][-1][a].all() and int(want["parked_calls"][-1].sum()) == len(a)
    assert want["starts"] == N + 37 + N                                              # the parking move is counted like any reset


def test_the_model_is_the_plain_one_where_nothing_parks():
    """Every reseed at depth 0 (the twin's script): ParkingModel's outputs are ScenarioModel's, byte for byte."""
    sc = rl.scenario("short", "GoToLocal", 65)
    ev = rl.twin_events(sc.events)
    got = rl.ParkingModel("GoToLocal", sc.seeds).run(ev)
    want = su.ScenarioModel("GoToLocal", sc.seeds).run([e[:3] if e[0] == "reseed" else e for e in ev])
    assert not got["parked"].any() and got["starts"] == want["starts"]
    for k, v in want["steps"].items():
        assert np.array_equal(su._bits(got["steps"][k]), su._bits(v)), k
    short = rl.model_run("short", "GoToLocal", 65)
    live = ~short["parked"]
    for k in ("image", "direction", "tokens", "done", "reward64"):
        assert np.array_equal(su._bits(short["steps"][k])[live], su._bits(want["steps"][k])[live]), k          # ... and a short env's until it parks


# ---- the argument --------------------------------------------------------------------------------------------------------------------
class _Lib(object):
    def __init__(self):
        self.option, self.calls = 0, []

    def bbai_reseed(self, handle, *a):
        self.calls.append(self.option)
        return 0


def _bare_env(n=8):
    """tests/test_binding_host.py::_bare_env with a recording library behind reseed's three calls."""
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv

    class Bare(BatchedBabyAIEnv):
        def get_option(self, name):
            assert name == "reseed_levels"
            return self.lib.option

        def set_option(self, name, value):
            assert name == "reseed_levels"
            self.lib.option = max(0, int(value))

        def _obs(self, rendered=False):
            return "obs"

        def _stream(self):
            return None

    env = Bare.__new__(Bare)
    env.torch, env.num_envs, env.device, env.handle, env.lib, env._hold = torch, n, torch.device("cpu"), None, _Lib(), {}
    env.image = env.direction = torch.zeros(1, dtype=torch.uint8)
    return env


def test_reseed_levels_argument():
    env = _bare_env()
    for bad in (-1, -7, 1.0, 2.5, "1", True, np.float32(1), [1]):
        with pytest.raises(ValueError, match="levels"):
            env.reseed([1, 2], [5, 6], levels=bad)
    assert env.lib.calls == []
    assert env.reseed([1, 2], [5, 6]) == "obs" and env.lib.calls == [0]                  # None: the option as it stands ...
    env.lib.option = 3
    env.reseed([1, 2], [5, 6], levels=None)
    assert env.lib.calls == [0, 3] and env.lib.option == 3
    for k in (1, np.int64(2), 0, 3, 10 ** 6):                                            # an int: for this call, the previous value back behind it
        env.reseed([1, 2], [5, 6], levels=k)
        assert env.lib.calls[-1] == int(k) and env.lib.option == 3
    with pytest.raises(ValueError, match="twice"):                                       # the other checks come behind it, unchanged
        env.reseed([1, 1], [5, 6], levels=1)
    assert env.reseed([], [], levels=2) == "obs" and env.lib.option == 3


def test_levels_argument_of_the_callers():
    from babyai_amd.engine import reseed_levels_arg
    from babyai_amd.evaluate import evaluate_policy
    from babyai_amd.imitation import DemoStore
    assert reseed_levels_arg(None, "t") is None and reseed_levels_arg(np.int32(4), "t") == 4 and reseed_levels_arg(0, "t") == 0
    with pytest.raises(ValueError, match="negative"):
        evaluate_policy(None, "BabyAI-GoToLocal-v0", 0, 4, pool=2, reseed_levels=-1)
    with pytest.raises(ValueError, match="integer"):
        DemoStore.collect_seeds("BabyAI-GoToLocal-v0", [1, 2], reseed_levels=1.5)
    with pytest.raises(ValueError, match="pool= serves tensor policies only"):           # the refusal stays
        evaluate_policy(None, "BabyAI-GoToLocal-v0", 0, 4, pool=2, agent=object(), reseed_levels=1)


# ---- the pool schedulers on the host build ---------------------------------------------------------------------------------------------
def _policy(obs, t):
    """A pure function of the observation: forward unless the cell ahead is not empty, then a turn chosen by the view's bytes."""
    import torch
    img = obs["image"].to(torch.int64)
    ahead = img[:, 3, 5, 0]
    turn = (img.reshape(img.shape[0], -1).sum(1) + obs["direction"].to(torch.int64)) % 2
    return torch.where(ahead == 1, torch.full_like(turn, 2), turn).to(torch.uint8)


def _episode(level, seed, limit=10 ** 6):
    """(frames, return) of env.seed(seed); env.reset() under _policy, one HostBatch of one env."""
    import torch
    from hostsim_util import HostBatch
    from babyai_amd.levels import make_cfg
    hb = HostBatch(make_cfg(level), [seed], auto_reset=False)
    hb.reset()
    for t in range(1, limit):
        a = _policy({"image": torch.as_tensor(hb.image), "direction": torch.as_tensor(hb.direction)}, t)
        hb.step(a.numpy())
        if hb.done[0]:
            return t, float(hb.reward64[0])


@pytest.mark.parametrize("level,episodes,pool,poll", [("GoToLocal", 40, 8, 16), ("GoToLocal", 23, 5, 3), ("GoToObjMaze", 10, 4, 16)])
def test_pool_evaluation_with_one_level_per_reseed_logs_the_same(level, episodes, pool, poll):
    from babyai_amd.evaluate import _evaluate_pool
    name, seed = "BabyAI-%s-v0" % level, 31000
    logs = {}
    for k in (None, 1, 2):
        del rl.HostEvalEnv.made[:]
        logs[k] = _evaluate_pool(_policy, name, seed, episodes, False, "cpu", pool, poll, reseed_levels=k, make_env=rl.HostEvalEnv)
        env, = rl.HostEvalEnv.made
        assert env.closed and env.levels_seen and set(env.levels_seen) == {k}
        assert not env.model.parked.any()          # auto_reset=False: an env freezes at its level's end and is reseeded, never moved on
    assert logs[1] == logs[None] == logs[2]
    want = [_episode(level, seed + j) for j in range(episodes)]
    assert logs[1]["num_frames_per_episode"] == [f for f, _ in want] and logs[1]["return_per_episode"] == [r for _, r in want]
    assert logs[1]["seed_per_episode"] == list(range(seed, seed + episodes))


@pytest.mark.parametrize("case", ["PickupDist", "BossLevel"])
def test_collect_seeds_with_one_level_per_reseed_returns_the_same(case):
    from babyai_amd.imitation import DemoStore
    level, (lo, hi), pool, chunk, kept, frames = sd.CASES[case]
    seeds = tuple(range(lo, hi))
    want = sd.expected(level, seeds)
    env0 = sd.HostPool(level, seeds[:pool])
    store0, kept0 = DemoStore.collect_seeds("BabyAI-%s-v0" % level, seeds, pool=pool, chunk=chunk, env=env0)
    for k in (1, 2):
        env = rl.HostPoolLevels(level, seeds[:pool])
        store, kept_k = DemoStore.collect_seeds("BabyAI-%s-v0" % level, seeds, pool=pool, chunk=chunk, env=env, reseed_levels=k)
        assert env.reseeds == env0.reseeds and set(env.levels_seen) == {k}
        assert env.parked_rows > 0                  # envs did park, and their unwritten history rows said `done` all along
        sd.assert_store_is(store, kept_k, want)
        assert np.array_equal(kept_k, kept0) and len(kept_k) == kept
        for key in ("image", "direction", "action", "tokens", "offset"):
            assert np.array_equal(getattr(store, key).numpy(), getattr(store0, key).numpy()), key
    assert env.model.parked.any()                   # the list ran out: the idle envs end parked


def test_adapters_pass_levels_through_only_when_given():
    import torch
    from babyai_amd import vec_env

    class Stub(object):
        def reseed(self, *a, **kw):
            self.got = (a, kw)

            class M(list):
                def snapshot(self):
                    return self
            return {"image": torch.zeros((2, 7, 7, 3), dtype=torch.uint8), "direction": torch.tensor([1, 3], dtype=torch.uint8), "mission": M(["a", "b"])}

    for cls in (vec_env.BatchedParallelEnv, vec_env.BatchedManyEnvs):
        st = Stub()
        v = cls("BabyAI-GoToLocal-v0", 2, engine=st)
        v.reseed([1, -1], [41, 42])
        assert st.got == (([1, -1], [41, 42]), {})                          # an engine that knows no depth is called as ever
        obs = v.reseed([0], [7], levels=1)
        assert st.got == (([0], [7]), {"levels": 1}) and len(obs) == 2
