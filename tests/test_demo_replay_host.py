"""`DemoStore.replay` without a GPU: the host twins of k_demo_replay_feed and k_demo_replay_judge against plain loops on synthetic pools, and the
whole loop with the host build as its `env=` against one plain model -- a single HostEnv per demo, reset and stepped with the demo's actions
(demo_replay_util.model: no pool, no hold, no reseed) -- on the expert's demonstrations, on stores made wrong on purpose and on a store of
random-action episodes.  The figures of the cases (demos, frames, which shifted seeds end early) are those of the issue, recomputed here."""
import numpy as np
import pytest
import torch

import demo_replay_util as ru
from babyai_amd.imitation import DemoReplay, DemoStore


# ---- replay_feed ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ru.FEED_POOLS)
def test_feed_twin_equals_the_plain_loop(n):
    case = ru.feed_case(n)
    assert case["phases"] == set(range(16))                       # the store's frames lie at every byte phase of 147 f
    if n >= 63:
        assert case["kinds"] >= {"byte0", "byte146", "dir", "tok0", "tok_later", "two_bytes", "at0"}
        c0 = case["calls"][0]
        for nm in ("idle", "used_up", "negative_pos", "job_beyond", "job_huge"):
            assert c0["fed"][c0["roles"][nm]] == 0 and c0["actions"][c0["roles"][nm]] == ru.HOLD
    last = case["calls"][-1]["results"]
    assert (last["mismatches"] > 0).any() and (last["mismatches"] == 0).any() and (last["first_mismatch"] > 0).any() or n == 1
    ru.assert_feed(case, ru.feed_run(case, "cpu"))


def test_feed_planted_differences_are_found_one_by_one():
    """In the first call of the 200-env pool: byte 0, byte 146 and the direction each give one mismatch at the env's frame; a token difference
    gives mission_ok = 0 at pos == 0 and nothing at pos > 0; the env at pos == 0 without a difference gives mission_ok = 1."""
    case = ru.feed_case(200)
    c, res = case["calls"][0], case["calls"][0]["results"]
    for nm in ("byte0", "byte146", "dir", "two_bytes"):
        i = c["roles"][nm]
        if c["fed"][i]:
            assert res["mismatches"][c["job"][i]] == 1 and res["first_mismatch"][c["job"][i]] == c["pos"][i], nm
    for nm, ok in (("tok0", 0), ("at0", 1)):
        i = c["roles"][nm]
        if c["fed"][i]:
            assert res["mission_ok"][c["job"][i]] == ok and res["mismatches"][c["job"][i]] == 0, nm
    i = c["roles"]["tok_later"]
    if c["fed"][i]:
        assert c["pos"][i] > 0 and res["mismatches"][c["job"][i]] == 0 and res["mission_ok"][c["job"][i]] == 0        # (never written: still its initial 0)


# ---- replay_judge -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ru.JUDGE_POOLS)
def test_judge_twin_equals_the_plain_loop(n):
    case = ru.judge_case(n)
    calls = case["calls"]
    if n >= 63:
        assert any((c["done"] != 0)[c["fed"] == 0].any() and (c["done"] != 0)[c["fed"] != 0].any() for c in calls)           # done on fed and on unfed envs
        used_up = [c for c in calls if (c["fin"] & (c["done"] == 0)).any()]
        assert used_up                                                  # a demo used up without done
        ran_out = [c for c in calls if c["claim"] and (c["ids"] >= 0).any() and ((c["job"] < 0) & (c["ids"] < 0)).any() and c["before"]["counters"][0] < case["J"]]
        assert ran_out                                                  # the list runs out in the middle of a call
        assert calls[-1]["counters"][0] > case["J"]                    # ... and the cursor ends above it
        assert (calls[-1]["results"]["played"] == -5).any()            # demos nobody played are untouched
    ru.assert_judge_equal(case, ru.judge_run(case, "cpu"))
    ru.assert_judge_equal(case, ru.judge_run(case, "cpu", carry=False))


# ---- the whole loop on the host build --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ru.LOOP_CASES))
def test_replay_of_expert_demos_is_exact(name):
    level, seeds, arrays = ru.expert_case(name)
    want = ru.model_store(level, seeds, arrays)
    lens = np.diff(arrays["offset"])
    assert np.array_equal(want["played"], lens) and np.array_equal(want["done_at"], lens) and (want["return64"] > 0).all()
    if name == "GoToLocal":
        assert lens.min() == 1 and lens.max() == 13
    if name == "BossLevel":
        assert lens.min() == 10 and lens.max() == 215
    for pool in (1, 7, 64):
        for r in (1, 3):
            rep, env = ru.host_replay(level, seeds, arrays, pool, reseed_every=r, poll_every=5)
            exact = ru.assert_replay_is(rep, want, arrays)
            assert exact.all() and env.num_envs == min(pool, len(seeds)) and env.stepped_envs == int(lens.sum())
            assert (env.reseeds == 0) == (pool == 64)
    logs = rep.logs()
    assert logs["num_frames_per_episode"] == lens.tolist() and logs["return_per_episode"] == want["return64"].tolist()
    assert logs["seed_per_episode"] == [int(s) for s in seeds] and isinstance(rep, DemoReplay)


def test_replay_results_do_not_depend_on_poll_every():
    level, seeds, arrays = ru.expert_case("PutNextLocal")
    want = ru.model_store(level, seeds, arrays)
    for poll in (1, 16, 1000):
        rep, _ = ru.host_replay(level, seeds, arrays, 5, reseed_every=2, poll_every=poll)
        ru.assert_replay_is(rep, want, arrays)


# ---- stores that are wrong -----------------------------------------------------------------------------------------------------------
def _check(level, seeds, arrays, pool=5, r=2):
    want = ru.model_store(level, seeds, arrays)
    rep, _ = ru.host_replay(level, seeds, arrays, pool, reseed_every=r, poll_every=3)
    return want, ru.assert_replay_is(rep, want, arrays)


def test_one_image_byte_flipped():
    level, seeds, arrays = ru.expert_case("PutNextLocal")
    a = int(np.argmax(np.diff(arrays["offset"])))
    k = int(np.diff(arrays["offset"])[a]) - 2
    image = arrays["image"].copy()
    image[arrays["offset"][a] + k, 6, 6, 2] ^= 0x40
    want, exact = _check(level, seeds, ru.edited(arrays, image=image))
    assert want["mismatches"][a] == 1 and want["first_mismatch"][a] == k and k > 0
    assert not exact[a] and np.delete(exact, a).all()


@pytest.mark.parametrize("name", sorted(ru.LOOP_CASES))
def test_every_seed_shifted_by_one(name):
    level, seeds, arrays = ru.expert_case(name)
    off = arrays["offset"]
    first = {k: (v[:12] if k == "tokens" else v[:13] if k == "offset" else v[:off[12]]) for k, v in arrays.items()}          # demos 0..11
    shifted = seeds[:12] + np.uint64(1)
    want, exact = _check(level, shifted, first)
    lens = np.diff(first["offset"])
    assert (want["first_mismatch"] == 0).all() and not exact.any()
    early = np.flatnonzero(want["done_at"] != 0)
    assert (want["done_at"][early] < lens[early]).all() or name != "GoToLocal"
    if name == "GoToLocal":                     # both kinds occur: two replays end early, the others run the demo out
        assert early.tolist() == [2, 11] and shifted[early].tolist() == [1003, 1012] and want["done_at"][early].tolist() == [2, 2]
        assert (want["played"][early] == 2).all() and (np.delete(want["played"], early) == np.delete(lens, early)).all()


def test_one_action_replaced_in_mid_demo():
    level, seeds, arrays = ru.expert_case("PutNextLocal")
    lens = np.diff(arrays["offset"])
    a = int(np.argmax(lens))
    action = arrays["action"].copy()
    at = arrays["offset"][a] + lens[a] // 2
    action[at] = 0 if action[at] != 0 else 1
    want, exact = _check(level, seeds, ru.edited(arrays, action=action))
    assert not exact[a] and np.delete(exact, a).all()
    assert want["first_mismatch"][a] == lens[a] // 2 + 1              # the frame behind the replaced action is the first that differs


def test_a_demo_cut_short_and_a_demo_with_frames_appended():
    level, seeds, arrays = ru.expert_case("GoToLocal")
    lens = np.diff(arrays["offset"])
    a = int(np.argmax(lens))
    want, exact = _check(level, seeds, ru.resized(arrays, a, -1))
    assert want["done_at"][a] == 0 and want["played"][a] == lens[a] - 1 and want["return64"][a] == 0.0 and want["mismatches"][a] == 0
    assert not exact[a] and np.delete(exact, a).all()
    want, exact = _check(level, seeds, ru.resized(arrays, a, 3))
    assert want["done_at"][a] == lens[a] and want["played"][a] == lens[a] and want["mismatches"][a] == 0 and want["return64"][a] > 0
    assert not exact[a] and np.delete(exact, a).all()                 # (done_at != the store's length)


def test_a_mission_token_changed():
    level, seeds, arrays = ru.expert_case("PutNextLocal")
    tokens = arrays["tokens"].copy()
    tokens[4, 1] ^= 1
    want, exact = _check(level, seeds, ru.edited(arrays, tokens=tokens))
    assert want["mission_ok"][4] == 0 and want["mismatches"][4] == 0 and want["done_at"][4] == np.diff(arrays["offset"])[4]
    assert not exact[4] and np.delete(exact, 4).all()


def test_a_zero_length_demo_in_mid_store():
    level, seeds, arrays = ru.expert_case("GoToLocal")
    with_empty = ru.with_empty_demo(arrays, 9)
    seeds2 = np.insert(seeds, 9, np.uint64(77))
    for pool in (3, 64):
        want, exact = _check(level, seeds2, with_empty, pool=pool)
        assert want["played"][9] == 0 and want["done_at"][9] == 0 and want["first_mismatch"][9] == -1 and want["mission_ok"][9] == 0
        assert np.delete(exact, 9).all() and len(exact) == 25 and exact[9] == (want["mission_ok"][9] != 0)
    only = {"image": arrays["image"][:0], "direction": arrays["direction"][:0], "action": arrays["action"][:0],
            "tokens": arrays["tokens"][:2], "offset": np.zeros(3, np.int64)}
    rep = ru.as_store(only).replay("BabyAI-GoToLocal-v0", [1, 2], env=None, device="cpu")          # nothing to play: no pool is made
    assert rep.played.tolist() == [0, 0] and rep.first_mismatch.tolist() == [-1, -1] and not rep.exact.any()


# ---- a store that is not the expert's ------------------------------------------------------------------------------------------------
def test_random_action_episodes_replay_exactly():
    level, seeds, arrays, returns = ru.random_case()
    for s in seeds[:24]:                        # the expert gives up on every seed of this level: collect_seeds cannot make such a store
        assert ru.sd.seed_episode(level, int(s))[0] is False
    want = ru.model_store(level, seeds, arrays)
    lens = np.diff(arrays["offset"])
    assert np.array_equal(want["done_at"], lens) and np.array_equal(want["return64"], returns)
    assert (returns == 0).sum() > len(returns) // 2                   # most end at max_steps
    for pool, r in ((1, 1), (7, 3), (64, 1)):
        rep, _ = ru.host_replay(level, seeds, arrays, pool, reseed_every=r)
        assert ru.assert_replay_is(rep, want, arrays).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
class _NeverDone(object):
    """A stand-in pool whose envs never report `done`."""

    def __init__(self, n):
        self.num_envs, self.device = n, torch.device("cpu")
        self.image, self.direction = torch.zeros((n, 7, 7, 3), dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8)
        self.reward64, self.done = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.uint8)
        self.instr = torch.zeros((n, 72), dtype=torch.uint8)
        self.steps = 0

    def step(self, actions):
        self.steps += 1

    def reseed(self, ids, seeds, levels=None):
        pass

    def close(self):
        raise AssertionError("the caller's pool stays the caller's")


def test_refusals():
    level, seeds, arrays = ru.expert_case("GoToLocal")
    store = ru.as_store(arrays)
    with pytest.raises(ValueError, match="seeds"):
        store.replay("BabyAI-GoToLocal-v0", seeds[:-1], env=ru.HostReplayPool(level, seeds[:3]))
    with pytest.raises(ValueError, match="done-action"):
        store.replay("BabyAI-GoToLocal-v0", seeds, env=ru.HostReplayPool(level, seeds[:3], done_actions=True))
    with pytest.raises(ValueError, match="at least 1"):
        store.replay("BabyAI-GoToLocal-v0", seeds, env=ru.HostReplayPool(level, seeds[:3]), reseed_every=0)


def test_a_pool_that_never_reports_done_runs_every_demo_out():
    """No `done` ever: every demo is used up, which finishes it too (played = its length, done_at = 0) -- well inside the tick budget."""
    level, seeds, arrays = ru.expert_case("GoToLocal")
    lens = np.diff(arrays["offset"])
    pool = _NeverDone(4)
    rep = ru.as_store(arrays).replay("BabyAI-GoToLocal-v0", seeds, env=pool, reseed_every=2, poll_every=4)
    assert np.array_equal(rep.played.numpy(), lens) and (rep.done_at == 0).all() and (rep.return64 == 0).all() and not rep.exact.any()
    assert pool.steps <= (-(-len(seeds) // 4) + 1) * (int(lens.max()) + 2) + 4


def test_the_tick_budget_ends_a_loop_that_makes_no_progress(monkeypatch):
    """The loop never spins: with the stand-in pool that never reports `done` and a judge that loses every result (a used-up demo finishes
    without `done`, so only a judge that does nothing keeps the counters still), the loop raises after exactly its budget of ticks."""
    import babyai_amd.imitation as im
    level, seeds, arrays = ru.expert_case("GoToLocal")
    lens = np.diff(arrays["offset"])
    monkeypatch.setattr(im, "replay_judge", lambda *a, **k: None)
    pool = _NeverDone(4)
    with pytest.raises(RuntimeError, match="ticks"):
        ru.as_store(arrays).replay("BabyAI-GoToLocal-v0", seeds, env=pool, reseed_every=2, poll_every=4)
    assert pool.steps == (-(-len(seeds) // 4) + 1) * (int(lens.max()) + 2) + 4
