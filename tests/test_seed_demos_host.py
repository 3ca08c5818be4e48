"""Expert demonstrations for LISTED seeds, a store that grows, and the loop that uses both (scripts/train_intelligent_expert.py:106-176), without a
GPU: the host twins of k_demo_jobs and k_demo_pack_list against plain loops, `DemoStore.collect_seeds` with the host build as its env against
one-env, one-seed episodes (HostEnv + HostBot: no pool, no ring, no scheduler) and against the demonstrations recorded from the reference's own
script, and `DemoStore.extend` against `from_reference` of the concatenation.  The figures in the case table (kept / dropped / frames) are those
of the issue; every one is recomputed here and asserted."""
import numpy as np
import pytest
import torch

import imitation_util as iu
import seed_demos_util as sd
from babyai_amd.imitation import DemoStore, collect_chunk


# ---- demo_jobs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,chunk,p_done", sd.JOBS_CASES, ids=["n%d-chunk%d-p%s" % c for c in sd.JOBS_CASES])
def test_jobs_twin_equals_the_plain_loop(n, chunk, p_done):
    case = sd.jobs_case(n, chunk, p_done)
    got = sd.jobs_run(case, chunk, "cpu")
    for c, (g, w) in enumerate(zip(got, case["want"])):
        for k in ("ids", "rec", "job", "start", "counters"):
            assert np.array_equal(g[k], w[k]), (c, k, g[k], w[k])
        claimed = w["ids"] >= 0
        assert np.array_equal(g["seeds"][claimed], w["seeds"][claimed]), c


def test_jobs_cases_reach_what_they_claim():
    """done on a chunk's first and last row, gave_up rows, reward == 0 rows, idle envs, a list that runs out in mid-call, kept and dropped episodes"""
    for n, chunk, p in sd.JOBS_CASES:
        case = sd.jobs_case(n, chunk, p)
        if n >= 63:                             # (n = 1 is the one-lane pool: a done on the chunk's first row only)
            for ch in case["chunks"]:
                assert ch["done"][0].any() and ch["done"][-1].any()
            assert (case["job0"] < 0).any() and any((ch["gave_up"] != 0).any() for ch in case["chunks"])
            assert any(((ch["done"] != 0) & (ch["reward"] == 0) & (ch["gave_up"] == 0)).any() for ch in case["chunks"])
            last = case["want"][-1]
            assert last["counters"][0] > case["J"] and (last["job"] == -1).sum() > (case["job0"] == -1).sum()
            ran_out = [c for c, w in enumerate(case["want"]) if (w["fin"] & (w["ids"] >= 0)).any() and (w["fin"] & (w["ids"] < 0)).any()]
            assert ran_out, (n, chunk, p)
            total = sum(len(w["rec"]) for w in case["want"])
            assert 0 < total < last["counters"][1]


# ---- demo_pack_list -----------------------------------------------------------------------------------------------------------------
LIST = {"wrap": (1, 3, 4, 5, [1, 2, 4, 5, 8, 9, 12, 3, 7, 1, 11, 12]), "one_slot": (2, 1, 6, 3, [1, 6, 2, 6, 3]),
        "many": (3, 4, 16, 70, list(np.random.default_rng(5).integers(1, 65, size=90)))}


@pytest.mark.parametrize("name", sorted(LIST))
def test_list_pack_twin_equals_direct_indexing(name):
    seed, R, T, n, lens = LIST[name]
    case = sd.ListCase(seed, R, T, n, lens)
    assert min(lens) == 1 and max(lens) == R * T or name == "many"
    if name == "wrap":
        assert case.wraps and case.slots_spanned.max() == R
    case.check(case.run("cpu"))


# ---- collect_seeds on the host build ----------------------------------------------------------------------------------------------------
def _collect(level, seeds, pool, chunk):
    env = sd.HostPool(level, seeds[:min(pool, len(seeds))])
    store, kept = DemoStore.collect_seeds("BabyAI-%s-v0" % level, seeds, chunk=chunk, env=env)
    assert not env.closed                       # (the caller's env stays the caller's)
    return store, kept, env


@pytest.mark.parametrize("name", sorted(sd.CASES))
def test_collect_seeds_equals_per_seed_episodes(name):
    level, (lo, hi), pool, chunk, n_kept, frames = sd.CASES[name]
    seeds = tuple(range(lo, hi))
    want = sd.expected(level, seeds)
    assert len(want["kept"]) == n_kept and (frames is None or int(want["offset"][-1]) == frames)
    lens = np.diff(want["offset"])
    if name == "PickupDist":
        assert want["gave_up"] == len(seeds) - n_kept == 19 and -(-int(lens.max()) // chunk) == 4
    if name == "UnlockToUnlock":
        assert len(seeds) - n_kept == 26
    store, kept, env = _collect(level, seeds, pool, chunk)
    sd.assert_store_is(store, kept, want)
    if name == "BossLevel":                     # demos that cross many slots
        assert -(-int(lens.max()) // chunk) >= 19
    assert env.reseeds >= 1


def test_collect_seeds_with_a_ring_that_wraps():
    """The level's step bound (8 x 64 x 9 = 4608 on BossLevel) gives a ring of 289 slots of 16 steps, which the 40 seeds above never fill.  An
    env object may state a tighter bound: here the longest episode of THIS list, so that the ring has as many slots as that episode needs
    plus one, the rounds go round it about twice, and the longest demo lies in all slots but one."""
    level, (lo, hi), pool, chunk, n_kept, frames = sd.CASES["BossLevel"]
    seeds = tuple(range(lo, hi))
    want = sd.expected(level, seeds)
    longest = max(len(sd.seed_episode(level, s)[4]) for s in seeds)
    env = sd.HostPool(level, seeds[:pool])
    env.max_steps_bound = longest
    store, kept = DemoStore.collect_seeds("BabyAI-BossLevel-v0", seeds, chunk=chunk, env=env)
    R = -(-longest // chunk) + 1
    assert R == 20 and env.rollouts >= 2 * R - 2
    sd.assert_store_is(store, kept, want)


def test_collect_seeds_pool_larger_than_the_list():
    level, seeds = "PickupDist", tuple(range(1000, 1020))
    env = sd.HostPool(level, seeds)
    store, kept = DemoStore.collect_seeds("BabyAI-PickupDist-v0", seeds, pool=4096, chunk=4, env=env)
    sd.assert_store_is(store, kept, sd.expected(level, seeds))
    assert env.reseeds == 0


def test_collect_seeds_shuffled_list_with_a_duplicate():
    level = "PickupDist"
    seeds = [int(s) for s in np.random.default_rng(3).permutation(np.arange(1000, 1040))]
    seeds.insert(17, seeds[2])
    seeds = tuple(seeds)
    want = sd.expected(level, seeds)
    store, kept, _ = _collect(level, seeds, 6, 4)
    sd.assert_store_is(store, kept, want)
    a, b = list(kept).index(2), list(kept).index(17)            # the duplicate yields an equal demonstration
    ref = store.to_reference()
    assert ref[a][0] == ref[b][0] and np.array_equal(ref[a][1], ref[b][1]) and ref[a][2:] == ref[b][2:]


def test_collect_seeds_empty_list():
    store, kept = DemoStore.collect_seeds("BabyAI-PickupDist-v0", [], env=sd.HostPool("PickupDist", [5]))
    assert len(store) == 0 and store.num_frames == 0 and kept.dtype == np.int64 and kept.shape == (0,)
    assert store.offset_host.tolist() == [0] and store.to_reference() == []


def test_collect_seeds_default_chunk_is_collects():
    assert collect_chunk(64) == 16 and collect_chunk(8 * 64 * 9) == 128 and collect_chunk(400) == 100 and collect_chunk(4608, 5) == 5


def done_mode_store(pool, chunk=16):
    """SynthSeq seeds 5..64 in the done-action mode on the host model."""
    seeds = tuple(range(5, 65))
    env = sd.HostPool("SynthSeq", seeds[:pool], done_actions=True)
    return DemoStore.collect_seeds("BabyAI-SynthSeq-v0", seeds, chunk=chunk, env=env)


def test_collect_seeds_in_done_action_mode_on_the_host_model():
    """The mode is the batch's: the pool (reseeds, lastStepMatch cleared per episode) gives what one env per seed gives, the expert ends its
    episodes with `done` actions, and the demonstrations differ from the mode-off ones."""
    (one, kept_one), (pool, kept_pool) = done_mode_store(60), done_mode_store(11)
    assert np.array_equal(kept_one, kept_pool) and 0 < len(kept_one) < 60
    _same_store(one, pool)
    off = sd.expected("SynthSeq", tuple(range(5, 65)))
    assert (pool.action == 6).any() and not (off["action"] == 6).any()
    assert any(" and " in d[0] for d in pool.to_reference())


# ---- the reference pin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", sd.GOLDEN_LEVELS)
def test_kept_demos_equal_the_reference_scripts(level):
    seeds = sd.golden_seeds(level)
    store, kept, _ = _collect(level, seeds, 5, 16)
    sd.assert_kept_equal_golden(level, store, kept)
    dropped = sorted(set(range(len(seeds))) - set(kept.tolist()))
    assert [seeds[j] for j in dropped] == sd.GOLDEN_DROPPED.get(level, [])
    sd.assert_store_is(store, kept, sd.expected(level, seeds))


def test_the_reference_pin_keeps_121_of_126():
    total = sum(len(sd.golden_seeds(lv)) for lv in sd.GOLDEN_LEVELS)
    kept = sum(len(sd.expected(lv, sd.golden_seeds(lv))["kept"]) for lv in sd.GOLDEN_LEVELS)
    assert (kept, total) == (121, 126)


# ---- extend -------------------------------------------------------------------------------------------------------------------------
def _demos(level):
    return iu.load_demos(level)


def _same_store(a, b):
    assert len(a) == len(b) and a.num_frames == b.num_frames
    assert np.array_equal(a.offset_host, b.offset_host) and torch.equal(a.offset, b.offset) and np.array_equal(a.lengths, b.lengths)
    for k in ("image", "direction", "action", "tokens"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_three_extends_equal_from_reference_of_the_concatenation(tmp_path):
    demos = _demos(iu.LEVELS[0]) + _demos(iu.LEVELS[1])
    cuts = [0, 3, 4, len(demos) // 2, len(demos)]
    store = DemoStore.from_reference(demos[cuts[0]:cuts[1]])
    for a, b in zip(cuts[1:], cuts[2:]):
        assert store.extend(DemoStore.from_reference(demos[a:b])) is store
    whole = DemoStore.from_reference(demos)
    _same_store(store, whole)
    assert store.image.shape == whole.image.shape and store.image.is_contiguous()
    order = np.random.default_rng(0).permutation(len(demos))[:9]
    _same_store(store.select(order), whole.select(order))
    x, y = store.batch(order), whole.batch(order)
    for k in ("image", "action", "done", "mask", "episode_ids", "inds", "instr"):
        assert torch.equal(getattr(x, k), getattr(y, k)), k
    assert np.array_equal(x.order, y.order) and np.array_equal(x.lengths, y.lengths)
    for (m1, i1, d1, a1), (m2, i2, d2, a2) in zip(store.to_reference(), whole.to_reference()):
        assert m1 == m2 and np.array_equal(i1, i2) and d1 == d2 and a1 == a2
    store.save(str(tmp_path / "s.npz"))
    _same_store(DemoStore.load(str(tmp_path / "s.npz")), whole)
    before = (len(store), store.capacity)
    store.extend(DemoStore.empty())                  # a no-op
    assert (len(store), store.capacity) == before
    _same_store(store, whole)


def test_extend_capacity_grows_geometrically():
    part = DemoStore.from_reference(_demos(iu.LEVELS[0])[:4])
    store = DemoStore.from_reference(_demos(iu.LEVELS[0])[:4])
    caps = [store.capacity]
    for _ in range(9):
        store.extend(part)
        caps.append(store.capacity)
        assert store.capacity[0] >= store.num_frames and store.capacity[1] >= len(store)
        assert store._buf["image"].numel() >= store.capacity[0] * 147 + 16         # 16 spare bytes behind the last frame
    grown = [(a, b) for a, b in zip(caps, caps[1:]) if a != b]
    for a, b in grown:
        assert (b[0] == a[0] or b[0] >= 2 * a[0]) and (b[1] == a[1] or b[1] >= 2 * a[1])
    assert caps[1] != caps[0]
    assert sum(1 for a, b in zip(caps[1:], caps[2:]) if a != b) <= 2             # eight equal extends after the first
    assert len(store) == 40 and np.array_equal(store.lengths, np.tile(part.lengths, 10))
    assert torch.equal(store.image, part.image.repeat(10, 1, 1, 1))


# ---- grow_training_set: the guard the reference lacks -------------------------------------------------------------------------------------
def test_grow_training_set_gives_up_under_a_learner_that_never_fails(monkeypatch):
    """scripts/train_intelligent_expert.py:162-174 loops for ever when no evaluation finds a failure; here max_rounds evaluations in a row that add
    nothing raise.  (The evaluation is replaced by its log; the loop itself against a plain restatement runs on the GPU.)"""
    from babyai_amd import evaluate, imitation
    calls = []

    def all_solved(policy, env_name, seed, episodes, **kw):
        calls.append(seed)
        return {"seed_per_episode": list(range(seed, seed + episodes)), "return_per_episode": [0.5] * episodes, "num_frames_per_episode": [3] * episodes}

    monkeypatch.setattr(evaluate, "evaluate_policy", all_solved)
    store = DemoStore.from_reference(_demos(iu.LEVELS[0])[:8])
    with pytest.raises(RuntimeError, match="added no demonstration"):
        imitation.grow_training_set(store, None, "BabyAI-GoToObjS4-v0", 7000, 2.0, 16, device="cpu", max_rounds=3)
    assert calls == [7000, 7016, 7032] and len(store) == 8
    assert imitation.grow_training_set(store, None, "BabyAI-GoToObjS4-v0", 7000, 1.0, 16, device="cpu") == 7000          # nothing to add: no evaluation
    assert calls == [7000, 7016, 7032]
