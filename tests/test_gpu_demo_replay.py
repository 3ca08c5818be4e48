"""k_demo_replay_feed, k_demo_replay_judge and `DemoStore.replay` on the device.  The kernels on the synthetic pools of
tests/test_demo_replay_host.py, against the same plain loops the host twins are held to; the whole loop against the one plain model
(demo_replay_util.model: a single HostEnv per demo) on the expert's demonstrations, on stores made wrong on purpose and on random-action
episodes; collect_seeds -> replay as a round trip; and what a replay leaves behind."""
import numpy as np
import pytest

import demo_replay_util as ru
import seed_demos_util as sd


@pytest.fixture(autouse=True)
def _clean_counters(monkeypatch):
    """Every engine batch a case closes -- the pools replay makes for itself included -- ends with gate_timeouts == 0 and no generator failure."""
    from babyai_amd.engine import BatchedBabyAIEnv
    seen, real = [], BatchedBabyAIEnv.close

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle:
            seen.append((self.get_option("gate_timeouts"), self.generator_failures()))
        real(self)

    monkeypatch.setattr(BatchedBabyAIEnv, "close", close)
    yield seen
    assert all(s == (0, 0) for s in seen), seen


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", ru.FEED_POOLS + (4099,))
def test_feed_kernel_equals_the_plain_loop(gpu, n):
    case = ru.feed_case(n)
    assert case["phases"] == set(range(16))
    ru.assert_feed(case, ru.feed_run(case, gpu))
    ru.assert_feed(case, ru.feed_run(case, "cpu"))          # ... which is what the twin gives


@pytest.mark.gpu
@pytest.mark.parametrize("n", ru.JUDGE_POOLS + (4099,))
def test_judge_kernel_equals_the_twin(gpu, n):
    """Scores, positions and counters must equal the plain loop's per env; the CLAIMS are compared as sets: the loop hands positions out in env
    order, the kernel wave by wave in whatever order the waves arrive, so every call starts from the loop's state in front of it.  A pool of
    one wave (n <= 64) claims in env order and also runs through its own carry, every field equal."""
    case = ru.judge_case(n)
    if n <= 64:
        ru.assert_judge_equal(case, ru.judge_run(case, gpu))
    J, job_demo, seeds = case["J"], case["job_demo"], case["job_seeds"]
    for c, (g, w) in enumerate(zip(ru.judge_run(case, gpu, carry=False), case["calls"])):
        assert np.array_equal(g["counters"], w["counters"]), (c, g["counters"], w["counters"])
        for k, v in w["results"].items():
            assert np.array_equal(g["results"][k].view(np.uint8), v.view(np.uint8)), (c, k)
        if not w["claim"]:
            assert np.array_equal(g["job"], w["job"]) and np.array_equal(g["pos"], w["pos"]) and np.array_equal(g["ids"], g["ids_before"]), c
            continue
        free = (w["before"]["job"] < 0) | w["fin"]                       # who claims: the same envs in both
        assert np.array_equal(g["job"][~free], w["job"][~free]) and np.array_equal(g["pos"][~free], w["pos"][~free]) and (g["ids"][~free] == -1).all()
        got = free & (g["ids"] >= 0)
        assert np.array_equal(g["ids"][got], np.flatnonzero(got)) and (g["ids"][free & ~got] == -1).all() and (g["job"][free & ~got] == -1).all()
        assert sorted(g["job"][got].tolist()) == sorted(w["job"][free & (w["ids"] >= 0)].tolist()), c          # the same demos handed out
        assert (g["pos"][got] == 0).all()
        k0 = int(w["before"]["counters"][0])
        order = np.argsort(g["job"][got])
        handed = np.arange(k0, min(J, k0 + int(free.sum())))
        by_demo = np.argsort(job_demo[handed])
        assert np.array_equal(g["job"][got][order], job_demo[handed][by_demo]) and np.array_equal(g["seeds"][got][order], seeds[handed][by_demo]), c
        if (free & ~got).any():
            assert g["counters"][0] > J


# ---- the whole loop ---------------------------------------------------------------------------------------------------------------------
def _replay(gpu, level, seeds, arrays, pool, r, **kw):
    return ru.as_store(arrays, gpu).replay("BabyAI-%s-v0" % level, seeds, device=gpu, pool=pool, reseed_every=r, **kw)


POOLS = ((1, 1), (65, 3), (4096, 1), (1, 3), (65, 1))         # (pool, reseed_every): pools 1, 65 and more than D


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ru.LOOP_CASES))
def test_replay_of_expert_demos_is_exact(gpu, name):
    level, seeds, arrays = ru.expert_case(name)
    want = ru.model_store(level, seeds, arrays)
    for pool, r in POOLS:
        rep = _replay(gpu, level, seeds, arrays, pool, r)
        assert rep.played.device == gpu
        assert ru.assert_replay_is(rep, want, arrays).all(), (pool, r)


@pytest.mark.gpu
def test_replay_of_wrong_stores(gpu):
    """The stores of tests/test_demo_replay_host.py's section 4, each against the model: a flipped image byte, shifted seeds, a replaced
    action, a demo cut short, a demo with frames appended, a changed mission token, a zero-length demo."""
    level, seeds, arrays = ru.expert_case("PutNextLocal")
    lens = np.diff(arrays["offset"])
    a = int(np.argmax(lens))
    image, action, tokens = arrays["image"].copy(), arrays["action"].copy(), arrays["tokens"].copy()
    image[arrays["offset"][a] + lens[a] - 2, 0, 0, 0] ^= 1
    action[arrays["offset"][a] + lens[a] // 2] ^= 1
    tokens[4, 1] ^= 1
    cases = [(seeds, ru.edited(arrays, image=image)), (seeds + np.uint64(1), arrays), (seeds, ru.edited(arrays, action=action)),
             (seeds, ru.resized(arrays, a, -1)), (seeds, ru.resized(arrays, a, 3)), (seeds, ru.edited(arrays, tokens=tokens)),
             (np.insert(seeds, 9, np.uint64(77)), ru.with_empty_demo(arrays, 9))]
    kinds = set()
    for k, (s, arr) in enumerate(cases):
        want = ru.model_store(level, s, arr)
        for pool, r in ((1, 1), (65, 3), (7, 2)):
            exact = ru.assert_replay_is(_replay(gpu, level, s, arr, pool, r), want, arr)
        assert not exact.all(), k
        kinds |= {"mismatch"} if (want["mismatches"] > 0).any() else set()
        kinds |= {"early"} if ((want["done_at"] > 0) & (want["done_at"] < np.diff(arr["offset"]))).any() else set()
        kinds |= {"no_done"} if ((want["done_at"] == 0) & (np.diff(arr["offset"]) > 0)).any() else set()
        kinds |= {"mission"} if ((want["mission_ok"] == 0) & (np.diff(arr["offset"]) > 0)).any() else set()
    assert kinds == {"mismatch", "early", "no_done", "mission"}


@pytest.mark.gpu
def test_goto_local_shifted_seeds_end_early_or_run_out(gpu):
    level, seeds, arrays = ru.expert_case("GoToLocal")
    shifted = seeds + np.uint64(1)
    want = ru.model_store(level, shifted, arrays)
    assert want["done_at"][2] == 2 and want["done_at"][11] == 2 and (want["done_at"] == 0).any()
    for pool, r in ((1, 1), (65, 3)):
        ru.assert_replay_is(_replay(gpu, level, shifted, arrays, pool, r), want, arrays)


@pytest.mark.gpu
def test_random_action_episodes_replay_exactly(gpu):
    level, seeds, arrays, returns = ru.random_case()
    want = ru.model_store(level, seeds, arrays)
    assert np.array_equal(want["return64"], returns) and (returns == 0).any()
    for pool, r in ((1, 1), (65, 3), (7, 1)):
        assert ru.assert_replay_is(_replay(gpu, level, seeds, arrays, pool, r), want, arrays).all()


@pytest.mark.gpu
def test_collect_seeds_then_replay(gpu):
    from babyai_amd.imitation import DemoStore
    level, (lo, hi), pool, chunk, n_kept, frames = sd.CASES["PickupDist"]
    seeds = np.arange(lo, hi, dtype=np.uint64)
    store, kept = DemoStore.collect_seeds("BabyAI-PickupDist-v0", seeds, device=gpu, pool=pool)
    assert len(store) == n_kept == 281 and store.num_frames == frames == 1416
    for p, r in ((37, 1), (65, 3)):
        rep = store.replay("BabyAI-PickupDist-v0", seeds[kept], device=gpu, pool=p, reseed_every=r)
        assert bool(rep.exact.all()) and bool((rep.return64 > 0).all()) and np.array_equal(rep.played.cpu().numpy(), store.lengths)
    logs = rep.logs()
    assert logs["seed_per_episode"] == seeds[kept].tolist() and len(logs["return_per_episode"]) == 281


# ---- what a replay leaves behind --------------------------------------------------------------------------------------------------------
def _fresh_owned(gpu):
    from babyai_amd.engine import BatchedBabyAIEnv
    env = BatchedBabyAIEnv("BabyAI-GoToLocal-v0", 8, device=gpu, seeds=5, auto_reset=False)
    try:
        env.enable_instr_tokens()
        env.reset()
        return env.get_option("owned")
    finally:
        env.close()


@pytest.mark.gpu
def test_a_replay_leaks_nothing_and_closes_its_pool(gpu, monkeypatch):
    import babyai_amd.imitation as im
    from babyai_amd.engine import BatchedBabyAIEnv
    level, seeds, arrays = ru.expert_case("GoToLocal")
    before = _fresh_owned(gpu)
    made, closed, real_init, real_close = [], [], BatchedBabyAIEnv.__init__, BatchedBabyAIEnv.close

    def init(self, *a, **k):
        real_init(self, *a, **k)
        made.append(self)

    def close(self):
        closed.append(self)
        real_close(self)

    monkeypatch.setattr(BatchedBabyAIEnv, "__init__", init)
    monkeypatch.setattr(BatchedBabyAIEnv, "close", close)
    _replay(gpu, level, seeds, arrays, 7, 2)
    assert len(made) == 1 and closed == made and not made[0].handle
    assert made[0].auto_reset is False and made[0].num_envs == 7

    def broken(*a, **k):
        raise KeyError("judge")

    monkeypatch.setattr(im, "replay_judge", broken)
    with pytest.raises(KeyError):
        _replay(gpu, level, seeds, arrays, 7, 2)
    assert len(made) == 2 and closed == made and not made[1].handle          # closed on an exception too
    monkeypatch.undo()
    assert _fresh_owned(gpu) == before


@pytest.mark.gpu
def test_the_entries_refuse_bad_arguments(gpu):
    """BBAI_ERR_ARG before any launch; n == 0 is a no-op."""
    import torch
    from babyai_amd.engine import EngineError
    from babyai_amd.imitation import replay_feed, replay_judge
    case = ru.feed_case(63)
    store = ru.as_store(case["arrays"], gpu)
    D = case["D"]
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=gpu)
    res = (z(D, torch.int32), z(D, torch.int32), z(D, torch.uint8))
    replay_feed(z((0, 7, 7, 3), torch.uint8), z(0, torch.uint8), z((0, 72), torch.uint8), z(0, torch.int32), z(0, torch.int32), store, *res,
                z(0, torch.uint8), z(0, torch.uint8))
    img = torch.zeros(2 * 147 + 1, dtype=torch.uint8, device=gpu)[1:].view(2, 7, 7, 3)          # a misaligned image array
    with pytest.raises(EngineError, match="aligned"):
        replay_feed(img, z(2, torch.uint8), z((2, 72), torch.uint8), z(2, torch.int32), z(2, torch.int32), store, *res, z(2, torch.uint8), z(2, torch.uint8))
    jc = ru.judge_case(63)
    off = torch.as_tensor(jc["offset"], device=gpu)
    replay_judge(z(0, torch.uint8), z(0, torch.uint8), z(0, torch.float64), z(0, torch.int32), z(0, torch.int32), off, z(jc["D"], torch.int32),
                 z(jc["D"], torch.int32), z(jc["D"], torch.float64), True, z(3, torch.int32), z(3, torch.int64), z(0, torch.int64), z(0, torch.int64),
                 z(2, torch.int64))
    torch.cuda.synchronize()
