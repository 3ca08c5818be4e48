"""k_demo_jobs, k_demo_pack_list, `DemoStore.collect_seeds` and `grow_training_set` on the device.  The kernels against their host twins (which
tests/test_seed_demos_host.py holds to plain loops) on the same synthetic inputs; collect_seeds against the per-seed episodes of the host build
(HostEnv + HostBot) and the demonstrations recorded from the reference's own script, byte for byte; against `DemoStore.collect` where every first
episode is solved; grow_training_set against a plain restatement from evaluate_policy and one-env batches.  BBAI_LOOKAHEAD=4 throughout: every
reseed then meets a ring that is consumed within a few steps."""
import numpy as np
import pytest

import seed_demos_util as sd


@pytest.fixture(autouse=True)
def _short_windows_and_clean_counters(monkeypatch):
    """BBAI_LOOKAHEAD=4, and every engine batch a case closes -- the ones collect_seeds, collect and evaluate_policy make for themselves
    included -- ends with gate_timeouts == 0 and generator_failures() == 0."""
    from babyai_amd.engine import BatchedBabyAIEnv
    monkeypatch.setenv("BBAI_LOOKAHEAD", "4")
    seen, real = [], BatchedBabyAIEnv.close

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle:
            seen.append((self.get_option("gate_timeouts"), self.generator_failures()))
        real(self)

    monkeypatch.setattr(BatchedBabyAIEnv, "close", close)
    yield seen
    assert all(s == (0, 0) for s in seen), seen


# ---- k_demo_jobs ------------------------------------------------------------------------------------------------------------------------
JOBS = sd.JOBS_CASES + [(4099, 4, 0.3), (4099, 16, 0.02)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,chunk,p_done", JOBS, ids=["n%d-chunk%d-p%s" % c for c in JOBS])
def test_jobs_kernel_equals_the_twin(gpu, n, chunk, p_done):
    """Which envs finished, their records and `start` must equal the twin's per env; the CLAIMS are compared as sets: the twin hands the jobs out
    in env order, the kernel wave by wave in whatever order the waves arrive.  Each call therefore starts from the twin's state in front of
    it; a pool of one wave (n <= 64) claims in env order and is also run through its own carry, every field equal."""
    case = sd.jobs_case(n, chunk, p_done)
    if n <= 64:
        for c, (g, w) in enumerate(zip(sd.jobs_run(case, chunk, gpu), case["want"])):
            for k in ("ids", "job", "start", "counters"):
                assert np.array_equal(g[k], w[k]), (c, k)
            assert np.array_equal(g["rec"][np.argsort(g["rec"][:, 0])], w["rec"]), c
    got = sd.jobs_run(case, chunk, gpu, carry=False)
    J, seeds = case["J"], case["seeds"]
    for c, (g, w) in enumerate(zip(got, case["want"])):
        assert np.array_equal(g["counters"], w["counters"]), (c, g["counters"], w["counters"])
        fin = w["fin"]
        # finished or not: ids_out >= 0 only on finished envs; an env that did not finish keeps its job and its start
        assert not (g["ids"][~fin] != -1).any() and np.array_equal(g["job"][~fin], g["job_before"][~fin]) and np.array_equal(g["start"][~fin], w["start"][~fin])
        # the records: the same rows in some order
        order = lambda r: r[np.argsort(r[:, 0], kind="stable")]
        assert np.array_equal(order(g["rec"]), order(w["rec"])), c
        # the claims: the same set of new jobs; every finished env holds exactly one of them, or -1 once the list is exhausted
        new_g, new_w = g["job"][fin], w["job"][fin]
        assert sorted(new_g[new_g >= 0].tolist()) == sorted(new_w[new_w >= 0].tolist()), c
        assert len(set(new_g[new_g >= 0].tolist())) == int((new_g >= 0).sum())
        if (new_g < 0).any():                   # only once the list is exhausted
            assert g["counters"][0] > J
        claimed = fin & (g["job"] >= 0)
        assert np.array_equal(np.flatnonzero(g["ids"] >= 0), np.flatnonzero(claimed)) and np.array_equal(g["ids"][claimed], np.flatnonzero(claimed))
        assert np.array_equal(g["seeds"][claimed], seeds[g["job"][claimed]])
        before = case["want"][c - 1]["start"] if c else np.zeros(n, np.int32)
        assert (g["start"][claimed] == (c + 1) * chunk).all() and np.array_equal(g["start"][fin & ~claimed], before[fin & ~claimed])


# ---- k_demo_pack_list -------------------------------------------------------------------------------------------------------------------
PACK_COUNTS = (1, 57, 58, 64, 65, 300)


@pytest.mark.gpu
@pytest.mark.parametrize("count", PACK_COUNTS)
def test_list_pack_kernel_one_frame_demos(gpu, count):
    """One-frame demos: an 8 KiB block of the image array then meets 57 runs, the most it can hold.  The sources lie at every byte phase."""
    case = sd.ListCase(100 + count, R=3, T=5, n=37, lens=[1] * count)
    import imitation_util as iu
    assert max(iu.runs_per_block(case.offset)) == (57 if count == 300 else min(count, 56))          # (a block that starts inside a frame meets 57)
    if count == 300:
        assert case.phases == set(range(16))
    assert (case.frames * sd.ROW) % 16 != 0 or count == 64           # the image array's last 16-byte chunk is short
    case.check(case.run(gpu))


@pytest.mark.gpu
@pytest.mark.parametrize("count", PACK_COUNTS)
def test_list_pack_kernel_wrapped_ring(gpu, count):
    """Demos of 1 frame up to R slots long whose first steps lie several turns into the ring."""
    R, T = 4, 6
    rng = np.random.default_rng(count)
    lens = rng.integers(1, R * T + 1, size=count)
    lens[0] = 1 if count > 1 else R * T
    lens[-1] = R * T
    case = sd.ListCase(200 + count, R, T, 41, lens)
    assert case.slots_spanned.max() == R and (count < 57 or (case.wraps and case.phases == set(range(16))))
    case.check(case.run(gpu))


@pytest.mark.gpu
def test_list_pack_twin_on_the_same_cases_is_what_the_kernel_is_held_to():
    """(The cases above compare the kernel with direct indexing; the twin is compared with direct indexing on the host.  One case through both.)"""
    case = sd.ListCase(7, 4, 6, 41, [1, 24, 3, 9])
    case.check(case.run("cpu"))


# ---- collect_seeds ------------------------------------------------------------------------------------------------------------------------
def _finish(env):
    assert env.get_option("gate_timeouts") == 0 and env.generator_failures() == 0


class _Watched(object):
    """A BatchedBabyAIEnv as collect_seeds' `env=`: the same calls passed on, and the counters every case ends with checked at close()."""

    def __init__(self, gpu, level, seeds, bound=None, **kw):
        from babyai_amd.engine import BatchedBabyAIEnv
        self.env = BatchedBabyAIEnv("BabyAI-%s-v0" % level, len(seeds), device=gpu, seeds=np.asarray(seeds, dtype=np.uint64), auto_reset=True, **kw)
        assert self.env.get_option("lookahead_period") == 4
        self.env.enable_instr_tokens()
        self.env.reset()
        self.num_envs, self.device = self.env.num_envs, self.env.device
        self.max_steps_bound = self.env.max_steps_bound if bound is None else bound
        self.rollouts = self.reseeds = 0

    def bot_rollout(self, steps, tokens=False, out=None):
        self.rollouts += 1
        return self.env.bot_rollout(steps, tokens=tokens, out=out)

    def reseed(self, ids, seeds):
        self.reseeds += 1
        return self.env.reseed(ids, seeds)

    def close(self):
        _finish(self.env)
        self.env.close()


def _collect(gpu, level, seeds, pool, chunk, bound=None, **kw):
    from babyai_amd.imitation import DemoStore
    env = _Watched(gpu, level, seeds[:min(pool, len(seeds))], bound=bound, **kw)
    try:
        store, kept = DemoStore.collect_seeds("BabyAI-%s-v0" % level, seeds, chunk=chunk, env=env)
    finally:
        env.close()
    assert store.device.type == "cuda"
    return store, kept, env


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(sd.CASES))
def test_collect_seeds_equals_the_host_results(gpu, name):
    level, (lo, hi), pool, chunk, n_kept, frames = sd.CASES[name]
    seeds = tuple(range(lo, hi))
    want = sd.expected(level, seeds)
    assert len(want["kept"]) == n_kept and (frames is None or int(want["offset"][-1]) == frames)
    store, kept, env = _collect(gpu, level, seeds, pool, chunk)
    sd.assert_store_is(store, kept, want)
    assert env.reseeds >= 1


@pytest.mark.gpu
def test_collect_seeds_with_a_ring_that_wraps(gpu):
    """tests/test_seed_demos_host.py's case of the same name: the ring sized by the longest episode of the list, gone round about twice."""
    level, (lo, hi), pool, chunk, _, _ = sd.CASES["BossLevel"]
    seeds = tuple(range(lo, hi))
    longest = max(len(sd.seed_episode(level, s)[4]) for s in seeds)
    store, kept, env = _collect(gpu, level, seeds, pool, chunk, bound=longest)
    assert env.rollouts >= 2 * (-(-longest // chunk) + 1) - 2
    sd.assert_store_is(store, kept, sd.expected(level, seeds))


@pytest.mark.gpu
def test_collect_seeds_pool_at_least_the_list_and_its_own_env(gpu, _short_windows_and_clean_counters):
    """pool >= len(seeds): one env per seed, no reseed -- through the public call, which makes, resets and closes its own env."""
    from babyai_amd.imitation import DemoStore
    level, seeds = "PickupDist", tuple(range(1000, 1300))
    store, kept = DemoStore.collect_seeds("BabyAI-PickupDist-v0", np.array(seeds), device=gpu, pool=4096)
    sd.assert_store_is(store, kept, sd.expected(level, seeds))
    store, kept = DemoStore.collect_seeds("BabyAI-PickupDist-v0", list(seeds), device=gpu, pool=64)          # ... and a pool, at the default chunk
    sd.assert_store_is(store, kept, sd.expected(level, seeds))
    store, kept = DemoStore.collect_seeds("BabyAI-PickupDist-v0", [], device=gpu)
    assert len(store) == 0 and kept.shape == (0,)
    assert len(_short_windows_and_clean_counters) == 2          # both batches were closed, and their counters read


@pytest.mark.gpu
def test_collect_seeds_in_done_action_mode(gpu):
    """SynthSeq seeds 5..64 with the batch in the reference's done-action mode, against the host model in that mode."""
    import torch
    from test_seed_demos_host import done_mode_store
    want, want_kept = done_mode_store(11)
    seeds = tuple(range(5, 65))
    store, kept, env = _collect(gpu, "SynthSeq", seeds, 11, 16, done_actions=True)
    assert np.array_equal(kept, want_kept) and np.array_equal(store.offset_host, want.offset_host)
    for k in ("image", "direction", "action", "tokens"):
        assert torch.equal(getattr(store, k).cpu(), getattr(want, k)), k
    assert (store.action == 6).any() and env.reseeds >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("level", sd.GOLDEN_LEVELS)
def test_kept_demos_equal_the_reference_scripts(gpu, level):
    seeds = sd.golden_seeds(level)
    store, kept, _ = _collect(gpu, level, seeds, 5, 16)
    sd.assert_kept_equal_golden(level, store, kept)
    assert [seeds[j] for j in sorted(set(range(len(seeds))) - set(kept.tolist()))] == sd.GOLDEN_DROPPED.get(level, [])
    sd.assert_store_is(store, kept, sd.expected(level, seeds))


@pytest.mark.gpu
@pytest.mark.parametrize("level,n,pool", [("GoToLocal", 300, 64), ("BossLevel", 200, 48)])
def test_collect_seeds_equals_collect_where_every_first_episode_is_solved(gpu, level, n, pool):
    """GoToLocal seeds 1000..1299 and BossLevel seeds 1000..1199: the expert solves the first episode of every stream, so "the first episode of
    stream seed + k that the expert solves" (collect) and "the episode seed + k starts, if solved" (collect_seeds) are the same demonstrations."""
    import torch
    from babyai_amd.imitation import DemoStore
    name = "BabyAI-%s-v0" % level
    want = DemoStore.collect(name, n, 1000, device=gpu)
    store, kept = DemoStore.collect_seeds(name, range(1000, 1000 + n), device=gpu, pool=pool)
    assert kept.tolist() == list(range(n)) and len(store) == n
    assert np.array_equal(store.offset_host, want.offset_host) and torch.equal(store.offset, want.offset)
    for k in ("image", "direction", "action", "tokens"):
        assert torch.equal(getattr(store, k), getattr(want, k)), k


# ---- grow_training_set ----------------------------------------------------------------------------------------------------------------------
def _policy(obs, t):
    """A fixed, stateless policy that often fails: it moves forward when the cell in front of the agent is empty (and sometimes when it is
    not) and turns otherwise, by a hash of the view -- a pure function of the observation."""
    import torch
    img = obs["image"].to(torch.int64)
    h = (img.reshape(img.shape[0], -1) * torch.arange(1, 148, device=img.device)).sum(1)
    front = img[:, 3, 5, 0]
    return torch.where((front == 1) & (h % 4 != 0), torch.full_like(h, 2), h % 2).to(torch.uint8)


@pytest.mark.gpu
def test_grow_training_set_equals_its_plain_restatement(gpu):
    import torch
    from babyai_amd.evaluate import evaluate_policy
    from babyai_amd.imitation import DemoStore, grow_training_set
    name, factor, per_round, eval_seed = "BabyAI-GoToLocal-v0", 1.5, 64, 5000
    store = DemoStore.collect(name, 40, 1000, device=gpu)
    plain = DemoStore.collect(name, 40, 1000, device=gpu)
    got_seed = grow_training_set(store, _policy, name, eval_seed, factor, per_round, device=gpu, pool=32)
    # train_intelligent_expert.py:150-176 with evaluate_policy and one env per listed seed, one batch per seed
    target, seed, rounds = int(40 * factor), eval_seed, 0
    while len(plain) < target:
        logs = evaluate_policy(_policy, name, seed, per_round, device=gpu)
        seed += per_round
        fails = [s for s, r in zip(logs["seed_per_episode"], logs["return_per_episode"]) if r <= 0][:target - len(plain)]
        for s in fails:
            one, kept = DemoStore.collect_seeds(name, [s], device=gpu, pool=1)
            assert len(one) == len(kept) <= 1
            plain.extend(one)
        rounds += 1
        assert rounds < 20
    assert 0 < len(fails) and len(plain) == target == 60
    assert got_seed == seed and len(store) == len(plain)
    assert np.array_equal(store.offset_host, plain.offset_host) and torch.equal(store.offset, plain.offset)
    for k in ("image", "direction", "action", "tokens"):
        assert torch.equal(getattr(store, k), getattr(plain, k)), k
    # the grown store is a store: batches and sub-stores come out of it as out of one built in one piece
    whole = DemoStore.from_reference(store.to_reference(), device=gpu)
    order = np.arange(len(store))[::-1].copy()
    x, y = store.batch(order), whole.batch(order)
    for k in ("image", "action", "done", "mask", "episode_ids", "inds", "instr"):
        assert torch.equal(getattr(x, k), getattr(y, k)), k
