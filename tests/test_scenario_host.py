"""tests/scenario_util.py without a GPU: the host model of bbai_reseed / bbai_save_state / bbai_load_state (ScenarioModel, the reference
tests/test_gpu_reseed_snapshot_entries.py holds the device to) against references it shares no code path with beyond the per-env host build --
HostEnv, a fresh HostBatch, the CPU oracle -- and, on the model alone, what every committed scenario claims to reach: events at the window
positions that matter, envs that finish on every tick behind a reseed, a state loaded one step from its time limit, one snapshot row in three
envs, the listed envs on the batch's edges and in the minority, and episodes that really end behind every event.

Two claims are not made everywhere, for reasons of the levels and not of the tests: a state one step from its time limit exists only where
max_steps (64 on GoToLocal, 100 to 1 152 elsewhere) fits a 140-step script; and the expert's BossLevel episodes outlast such a script, so that
scenario asks for one listed env per event with two finished episodes, not for every one."""
import numpy as np
import pytest

from babyai_amd.levels import make_cfg
from babyai_amd.missions import detokenize
from hostsim_util import HostBatch, HostEnv
import scenario_util as su

LEVELS = ["GoToLocal", "BossLevel", "PutNextS5N2Carrying"]
RESET_ENV = su.RESET_ENV


def _acts(T, n, seed, resets):
    return su._acts(T, n, seed, resets)


def _oracle(level, seed):
    from oracle import refenv
    from oracle import levels as olevels
    refenv.enable_shim()
    e = olevels.make_env(level)
    e.seed(int(seed))
    return e


# ---- the model against independent references -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
def test_a_reseeded_row_is_a_fresh_envs_reset_and_goes_on_as_a_fresh_batch(level):
    n, base = 24, 7100
    resets = 0.0 if level == "GoToLocal" else 0.08
    a, c = su.ScenarioModel(level, np.arange(n) + base), su.ScenarioModel(level, np.arange(n) + base)
    pre = _acts(22, n, 1, resets)
    for t in range(22):
        a.step(pre[t]); c.step(pre[t])
    ids = np.array([5, -1, 0, 23, n, 12, 17], dtype=np.int64)           # (-1 and n: skipped)
    seeds = su.new_seeds(len(ids), 31337)
    ok = (ids >= 0) & (ids < n)
    starts0 = a.starts
    a.reseed(ids, seeds)
    assert a.starts - starts0 == int(ok.sum())
    cfg = make_cfg(level)
    missions = a.missions()
    for i, s in zip(ids[ok], seeds[ok]):
        h = HostEnv(cfg, int(s))
        assert np.array_equal(a.hb.image[i], h.reset()), i
        assert a.hb.direction[i] == h.agent[2] and missions[i] == h.mission
        o = _oracle(level, s)
        want = o.reset()
        assert np.array_equal(a.hb.image[i], want["image"]) and a.hb.direction[i] == want["direction"] and missions[i] == want["mission"], (level, i)
        assert detokenize(a.tokens()[i]) == want["mission"]
    unl = np.setdiff1d(np.arange(n), ids[ok])
    for k in ("image", "direction", "rec", "hot", "stale", "mt", "mti"):
        assert np.array_equal(getattr(a.hb, k)[unl], getattr(c.hb, k)[unl]), k
    b = HostBatch(cfg, seeds[ok])
    b.reset()
    ab, aa = _acts(150, int(ok.sum()), 2, max(resets, 0.02)), _acts(150, n, 3, resets)
    aa[:, ids[ok]] = ab
    ends = np.zeros(int(ok.sum()), int)
    for t in range(150):
        a.step(aa[t]); c.step(aa[t]); b.step(ab[t])
        for k in su.OUT_KEYS:
            assert np.array_equal(su._bits(getattr(a.hb, k)[ids[ok]]), su._bits(getattr(b, k))), (level, t, k)
            assert np.array_equal(su._bits(getattr(a.hb, k)[unl]), su._bits(getattr(c.hb, k)[unl])), (level, t, k)
        ends += b.done
    assert ends.min() >= 2, ends          # (several levels of the new streams)


@pytest.mark.parametrize("auto_reset", [True, False], ids=["auto", "frozen"])
@pytest.mark.parametrize("level", LEVELS)
def test_a_loaded_env_continues_as_the_saved_one_and_keeps_its_own_next_level(level, auto_reset):
    n, base = 32, 7300
    a, c = (su.ScenarioModel(level, np.arange(n) + base, auto_reset=auto_reset) for _ in range(2))
    pre = _acts(10, n, 4, 0.0) % 6
    for t in range(10):
        a.step(pre[t]); c.step(pre[t])
    src = np.array([3, 9, 20, 31, n, 14], dtype=np.int64)
    dst = np.array([1, 8, 22, 0, 5, -1], dtype=np.int64)
    rows = np.array([0, 1, 2, 3, len(src), 5], dtype=np.int64)          # (a row outside the snapshot and env -1: skipped; snapshot row 4, of env n, stays zeroed)
    ok = (rows < len(src)) & (dst >= 0)
    saved_image = a.hb.image[src[ok]].copy()
    was_first = a.hb.step_count[src[ok]] == 0
    snap = a.save(src)
    assert np.array_equal(snap["rec"][ok], a.hb.rec[src[ok]]) and not snap["rec"][~(src < n)].any() and not snap["hot"][~(src < n)].any()
    other = _acts(6, n, 5, 0.0) % 6
    for t in range(6):                       # a diverges from c; the snapshot is not touched by it
        a.step(other[t])
    mt0, mti0 = a.hb.mt.copy(), a.hb.mti.copy()
    untouched = np.setdiff1d(np.arange(n), dst[ok])
    before = {k: getattr(a.hb, k)[untouched].copy() for k in ("image", "direction", "rec", "hot", "stale")}
    a.load(snap, dst, rows)
    assert np.array_equal(a.hb.mt, mt0) and np.array_equal(a.hb.mti, mti0)
    for k, v in before.items():
        assert np.array_equal(getattr(a.hb, k)[untouched], v), k
    keep = ~was_first | (level != "PutNextS5N2Carrying")     # (a start-carry level's reset() shows the state BEFORE the hand-over, a load the one after)
    assert np.array_equal(a.hb.image[dst[ok]][keep], saved_image[keep])
    assert np.array_equal(a.hb.rec[dst[ok]], snap["rec"][ok]) and np.array_equal(a.hb.hot[dst[ok], :15], snap["hot"][ok, :15])
    acts = _acts(80, n, 6, 0.0)
    inside = np.ones(int(ok.sum()), bool)                     # still inside the saved episode
    compared = 0
    for t in range(80):
        aa = acts[t].copy()
        aa[dst[ok]] = acts[t][src[ok]]
        a.step(aa); c.step(acts[t])
        for j, (s, d) in enumerate(zip(src[ok], dst[ok])):
            if not inside[j]:
                continue
            assert a.hb.reward64[d:d + 1].view(np.uint64)[0] == c.hb.reward64[s:s + 1].view(np.uint64)[0] and a.hb.done[d] == c.hb.done[s], (level, t, j)
            if c.hb.done[s]:
                inside[j] = False              # (the next level is the loaded env's OWN: another one than the saved env's)
                if not auto_reset:
                    assert np.array_equal(a.hb.image[d], c.hb.image[s])
            else:
                assert np.array_equal(a.hb.image[d], c.hb.image[s]) and a.hb.direction[d] == c.hb.direction[s], (level, t, j)
                compared += 1
    assert compared >= 40, compared


def test_a_loaded_envs_next_level_is_the_one_its_own_stream_had_next():
    """GoToLocal, 2 steps behind the reset: a loaded env, once the loaded episode ends, starts level 1 of ITS stream -- what a HostEnv of its seed
    gives at its second reset()."""
    n, base = 16, 7500
    a = su.ScenarioModel("GoToLocal", np.arange(n) + base)
    pre = _acts(2, n, 7, 0.0) % 3
    for t in range(2):
        a.step(pre[t])
    assert not a.hb.done.any() and a.starts == n
    snap = a.save([2, 3])
    a.load(snap, [10, 11, 12], [0, 1, 0])
    cmd = np.zeros(n, np.uint8)
    cmd[[10, 11, 12]] = RESET_ENV
    a.step(cmd)
    cfg = make_cfg("GoToLocal")
    for i in (10, 11, 12):
        h = HostEnv(cfg, base + i)
        h.reset()
        assert np.array_equal(a.hb.image[i], h.reset()) and a.missions()[i] == h.mission, i
    assert a.starts == n + 3


def test_the_expert_model_is_host_bot_on_host_env():
    """ScenarioModel.bot_decide against hostsim_util.HostBot driving HostEnv (what tests/test_hostsim_bot.py pins to the reference), 60 steps of
    GoToLocal across many episodes."""
    from hostsim_util import HostBot
    n, base = 12, 7700
    cfg = make_cfg("GoToLocal")
    a = su.ScenarioModel("GoToLocal", np.arange(n) + base)
    envs = [HostEnv(cfg, base + i) for i in range(n)]
    for e in envs:
        e.reset()
    bots = [HostBot(e) for e in envs]
    first = [True] * n
    episodes = 0
    for t in range(60):
        act, gave = a.bot_decide()
        a.step(act)
        for i, e in enumerate(envs):
            d = bots[i].decide(first[i])
            first[i] = False
            assert (RESET_ENV if d is None else d) == act[i] and bool(gave[i]) == (d is None), (t, i)
            if d is None:
                done, rew = True, 0.0
            else:
                _, rew, done = e.step(d)
            assert bool(a.hb.done[i]) == done and a.hb.reward[i] == np.float32(rew)
            if done:
                e.reset()
                first[i] = True
                episodes += 1
    assert episodes >= 3 * n


def _host_envs(level, seeds, pre):
    """One HostEnv per seed behind reset() and the steps pre[T, n] (auto-resetting, actions 0 .. 6): per-env objects that share no batch code
    with ScenarioModel."""
    cfg = make_cfg(level)
    envs = [HostEnv(cfg, int(s)) for s in seeds]
    for e in envs:
        e.reset()
    for t in range(len(pre)):
        for i, e in enumerate(envs):
            if e.step(int(pre[t, i]))[2]:
                e.reset()
    return envs


@pytest.mark.parametrize("with_rec", [True, False], ids=["records", "hot-only"])
@pytest.mark.parametrize("level", LEVELS)
def test_an_imported_range_continues_as_the_donor_rows_and_keeps_its_own_next_levels(level, with_rec):
    """The ("import", rows, first) event against per-env HostEnv objects: env first + k of the recipient gets donor row k's record, hot bytes
    0 .. 14 and stale set written into ITS object -- which keeps its own MT19937 stream --, is stepped on, and restarts through its own reset().
    With records: a donor row twice; the model's image / direction are what the last step wrote until the next step; the expert starts a fresh
    Bot on the imported rows, and only there.  Hot-only: the range's own poses with the direction turned -- valid for the records they stay
    with, since every direction is valid wherever the agent stands --, the expert's plans and the token rows untouched."""
    from hostsim_util import HostBot
    n, first, count = 24, 5, 9
    base_r, base_d = 7800, 8800
    pre_r, pre_d = _acts(12, n, 31, 0.0), _acts(12, n, 32, 0.0)
    a, c = (su.ScenarioModel(level, np.arange(n) + base_r) for _ in range(2))
    d = su.ScenarioModel(level, np.arange(n) + base_d)
    for t in range(12):
        a.step(pre_r[t]); c.step(pre_r[t]); d.step(pre_d[t])
    envs = _host_envs(level, np.arange(n) + base_r, pre_r)
    for i, e in enumerate(envs):
        assert np.array_equal(e.rec, a.hb.rec[i]) and np.array_equal(e.hot[:15], a.hb.hot[i, :15]) and e.stale.value == a.hb.stale[i]
    a.bot_decide(); c.bot_decide()                      # every env has a plan now (no env is fresh any more)
    assert not a._bot_fresh.any()
    if with_rec:
        src = np.array([3, 3, 0, 23, 11, 12, 13, 20, 7], dtype=np.int64)          # donor row 3 twice
        rows = {"rec": d.hb.rec[src].copy(), "hot": d.hb.hot[src].copy(), "stale": d.hb.stale[src].copy()}
        rows["hot"][:, 15] = 0xEE                        # (the exporter's ring slot: ignored)
    else:
        hot = a.hb.hot[first:first + count].copy()
        hot[:, 2] = (hot[:, 2] + 1 + np.arange(count) % 3) % 4
        rows = {"rec": None, "hot": hot, "stale": None}
    before = {k: getattr(a.hb, k).copy() for k in ("image", "direction", "mt", "mti", "rec", "hot", "stale")}
    tok0, starts0 = a.tokens(), a.starts
    a.import_state(rows, first)
    rng_ = np.arange(first, first + count)
    out = np.setdiff1d(np.arange(n), rng_)
    for k in ("image", "direction", "mt", "mti"):           # no observation is written; the level streams stay
        assert np.array_equal(getattr(a.hb, k), before[k]), k
    for k in ("rec", "hot", "stale"):
        assert np.array_equal(getattr(a.hb, k)[out], before[k][out]), k
    assert np.array_equal(a.hb.hot[:, 15], before["hot"][:, 15]) and a.starts == starts0
    assert np.array_equal(a._bot_fresh, np.isin(np.arange(n), rng_) & with_rec)
    if with_rec:
        assert np.array_equal(a.tokens()[rng_], d.tokens()[src]) and np.array_equal(a.tokens()[out], tok0[out])
        assert (a.tokens()[rng_] != tok0[rng_]).any()
    else:
        assert np.array_equal(a.tokens(), tok0) and np.array_equal(a.hb.rec, before["rec"])
    for k, i in enumerate(rng_):                          # the same bytes into the per-env objects
        if with_rec:
            envs[i].rec[:] = rows["rec"][k]
            envs[i].stale.value = int(rows["stale"][k])
        envs[i].hot[:14] = rows["hot"][k, :14]          # (byte 14, LevelGen.locked_room, belongs to the env's own level stream)
    # the expert: a fresh Bot on the imported rows (HostBot on the per-env object), the old plan's next decision elsewhere
    act, gave = a.bot_decide()
    act_c, _ = c.bot_decide()
    assert np.array_equal(act[out], act_c[out])
    if with_rec:
        for i in rng_:
            want = HostBot(envs[i]).decide(True)
            assert (RESET_ENV if want is None else want) == act[i] and bool(gave[i]) == (want is None), i
    acts = _acts(150, n, 33, 0.0)
    ends = np.zeros(n, int)
    for t in range(150):
        a.step(acts[t]); c.step(acts[t])
        for i, e in enumerate(envs):
            img, rew, done = e.step(int(acts[t, i]))
            assert bool(a.hb.done[i]) == done and a.hb.reward64[i:i + 1].view(np.uint64)[0] == np.float64(e.last_reward64).reshape(1).view(np.uint64)[0], (level, t, i)
            if done:
                img = e.reset()                          # ... its OWN next level
                ends[i] += 1
            assert np.array_equal(a.hb.image[i], img) and a.hb.direction[i] == e.agent[2], (level, t, i)
        for k in su.OUT_KEYS:
            assert np.array_equal(su._bits(getattr(a.hb, k)[out]), su._bits(getattr(c.hb, k)[out])), (level, t, k)
    if level == "GoToLocal":
        assert ends[rng_].min() >= 2, ends          # (64 steps at most per episode: two own levels behind the imported one)
    assert a.starts - starts0 == int(ends.sum())


def test_an_import_clears_the_done_action_byte():
    """Done-action mode: the model's lastStepMatch word of every imported env is cleared, also by a hot-only import, and nowhere else."""
    n = 16
    a = su.ScenarioModel("GoToLocal", np.arange(n) + 7950, done_actions=True)
    a.hb.lsm[:] = 1
    a.import_state({"rec": a.hb.rec[2:5].copy(), "hot": a.hb.hot[2:5].copy(), "stale": a.hb.stale[2:5].copy()}, 2)
    a.import_state({"rec": None, "hot": a.hb.hot[9:10].copy(), "stale": None}, 9)
    assert a.hb.lsm.tolist() == [int(i not in (2, 3, 4, 9)) for i in range(n)]


# ---- what the scripts of tests/test_gpu_state_ranges.py reach (tests/state_ranges_util.py, the model alone) ---------------------------------
def test_range_import_scripts_reach_the_recipients_own_next_levels():
    """Every case of test_range_import_steps_as_the_host_model: the import stands in front of the window position the case names, all four
    positions occur in every layout, and at least a quarter of the imported envs start a new episode -- of their OWN stream -- in the 30
    steps behind it.  A random walk does not finish a GoToLocal episode that soon (the donor rows are 20 steps into 64), so the reset command
    comes at scenario_util's rate on every level here."""
    import state_ranges_util as sr
    import test_gpu_state_ranges as tr
    assert len(tr.CASES2) == len(tr.IDS2) == len(set(tr.IDS2)) == 10 * len(sr.RANGES) + 4
    positions = {}
    for level, ev, ev_src, done_actions, first, count, pos, repeat in tr.CASES2:
        run = sr.import_run(level, first, count, pos, done_actions, False, repeat)
        log = [e for e in run["model"]["log"] if e["kind"] == "import"]
        assert len(log) == 1 and (log[0]["at"] + 1) % su.B == pos and log[0]["ids"] == list(range(first, first + count))
        assert run["model"]["T"] - log[0]["at"] == sr.AFTER
        assert int(run["restarted"].sum()) * 4 >= count, (level, first, count, int(run["restarted"].sum()))
        assert len(set(run["src"].tolist())) == count - (6 if repeat else 0)
        positions.setdefault((level, tuple(sorted(ev.items())), done_actions), set()).add(pos)
    assert all(p == set(range(su.B)) for p in positions.values())
    assert {(tuple(ev.items()), tuple(es.items())) for _, ev, es, _, _, _, _, _ in tr.CASES2 if ev != es} == \
        {((("BBAI_INPLACE", "1"),), (("BBAI_INPLACE", "0"),)), ((("BBAI_INPLACE", "0"),), (("BBAI_INPLACE", "1"),))}


def test_expert_import_case_has_colliding_pairs():
    """test_an_import_starts_a_fresh_expert: 33 of the 37 (row, env) pairs collide -- the row's Hot.step is the 10 the env's own plan expects
    and the env's own episode has not ended --, so a plan that survived the import would be continued; at least 8 are required.  The fresh
    decisions differ from the continued plans' somewhere, and the model's fresh decisions are HostBot's on the rows."""
    import state_ranges_util as sr
    from hostsim_util import HostBot
    case = sr.expert_case()
    assert int(case["colliding"].sum()) == 33 and int(case["colliding"].sum()) >= 8
    cfg = make_cfg(sr.BOT_LEVEL)
    for k in range(sr.BOT_COUNT):
        e = HostEnv(cfg, 0)
        e.rec[:], e.hot[:] = case["rows"]["rec"][k], case["rows"]["hot"][k]
        e.stale.value = int(case["rows"]["stale"][k])
        d = HostBot(e).decide(True)
        assert (255 if d is None else d) == case["want"][sr.BOT_FIRST + k], k
    out = np.setdiff1d(np.arange(sr.N), np.arange(sr.BOT_FIRST, sr.BOT_FIRST + sr.BOT_COUNT))
    assert np.array_equal(case["want"][out], case["want_twin"][out])
    assert (case["want"] != case["want_twin"]).any()


def test_done_action_import_case_meets_envs_in_front_of_their_target():
    import state_ranges_util as sr
    case = sr.done_case()
    m, pre = case["model"]["steps"], case["pre"]
    matched = sr.DONE_FIRST + np.nonzero(case["is_matched"])[0]
    assert len(matched) >= 1 and len(case["donor_acts"]) >= 20 and (case["donor_paid"] > 0).all()
    assert not m["reward64"][pre][matched].any() and m["done"][pre][sr.DONE_FIRST:sr.DONE_FIRST + sr.DONE_COUNT].all()
    assert (m["reward64"][pre + 1:] > 0).any()          # (later `done` actions do succeed: the mode is on)


@pytest.mark.parametrize("level", ["GoToLocal", "BossLevel"])
def test_pose_import_script_turns_agents_that_then_move(level):
    """The three imports without records stand in front of window positions 1, 3 and 0, and the turned agents' next steps differ from those of a
    run without the imports (the poses matter)."""
    import state_ranges_util as sr
    run = sr.pose_run(level)
    log = [e for e in run["model"]["log"] if e["kind"] == "import"]
    assert [(e["at"] + 1) % su.B for e in log] == [1, 3, 0] and not any(e["rec"] for e in log)
    assert [len(e["ids"]) for e in log] == [sr.POSE_COUNT, sr.N, 64]
    plain = su.ScenarioModel(level, sr.seeds(sr.RECIPIENT_SEED + 2000)).run(sr.twin_script(run["events"]))
    at = log[0]["at"]
    differ = (run["model"]["steps"]["image"][at] != plain["steps"]["image"][at]).reshape(sr.N, -1).any(1)
    assert differ[sr.POSE_FIRST:sr.POSE_FIRST + sr.POSE_COUNT].sum() >= sr.POSE_COUNT // 2 and not differ[:sr.POSE_FIRST].any()
    assert np.array_equal(run["model"]["steps"]["image"][:at], plain["steps"]["image"][:at])


# ---- what the committed scenarios reach (the model alone) -----------------------------------------------------------------------------------
def _edges(n):
    return {0, n - 1} | {b + d for b in range(64, n, 64) for d in (-1, 0)}


@pytest.mark.parametrize("name,level,n", su.COMMITTED, ids=["%s-%s-n%d" % c for c in su.COMMITTED])
def test_committed_scenario_reaches_what_it_claims(name, level, n):
    B = su.B
    sc, m = su.scenario(name, level, n), su.model_run(name, level, n)
    done, log = m["steps"]["done"], m["log"]
    assert 60 <= m["T"] <= 140
    assert {"fan3", "edges"} <= sc.claims and ("majority" in sc.claims or "every_env" in sc.claims)
    assert any(e["kind"] == "reseed" for e in log) and any(e["kind"] == "load" for e in log)
    listed = set()          # by any call: reseeded, saved or loaded
    for ev in sc.events:
        if ev[0] in ("reseed", "save", "load"):
            ids = ev[2 if ev[0] == "load" else 1]
            ids = list(range(n)) if ids is None else [int(i) for i in ids]
            assert len(set(ids)) == len(ids)          # (an env twice in one call is a caller error)
            if len(ids) < n:
                listed |= set(ids)
    if "two_episodes" in sc.claims or "one_episode" in sc.claims:
        for e in log:
            ends = done[e["at"]:, e["ids"]].sum(0)
            if "two_episodes" in sc.claims:
                assert ends.min() >= 2, (e["kind"], e["at"], ends)
            else:
                assert ends.max() >= 2 and np.median(ends) >= 1, (e["kind"], e["at"], ends)
    if "positions" in sc.claims:
        assert {(e["at"] + 1) % B for e in log if e["kind"] == "reseed"} >= {0, 1, B - 1}
        assert {(e["at"] + 1) % B for e in log if e["kind"] == "load"} - {0, B - 1}          # a load in mid-window
    if "every_tick" in sc.claims:
        full = False
        for env, s0, s1 in sc.info["every_tick"]:
            assert any(e["kind"] == "reseed" and e["at"] == s0 and env in e["ids"] for e in log)
            assert (s1 + 1) % B == 0 and done[s0:s1, env].all()          # a finish on every tick from the reseed to the window's last
            full |= s1 - s0 == B                                          # ... all B of them: B + 1 slots consumed in one window
        assert full
    if "time_limit" in sc.claims:
        hit = 0
        for e in log:
            if e["kind"] == "load":
                last = np.asarray(e["ids"])[e["step_count"] == e["max_steps"] - 1]
                hit += len(last)
                assert done[e["at"], last].all() and not m["steps"]["reward64"][e["at"], last].any()          # they time out on the very next tick
        assert hit >= 3
    for e in log:
        if e["kind"] == "load":
            assert not (sc.auto_reset and e["frozen"].any())          # (a frozen row makes a frozen env, which re-emits: for auto_reset=False only)
    assert any(e["kind"] == "load" and np.bincount(e["rows"]).max() >= 3 for e in log)          # fan3
    assert _edges(n) <= listed, sorted(_edges(n) - listed)
    assert len(listed) < n / 2          # (the calls that list envs; "every_env": one reseed besides takes the whole batch)
    assert ("every_env" in sc.claims) == any(e.get("all") for e in log)
    if "one_window" in sc.claims:
        assert len({(e["at"] + 1) // B for e in log}) == 1 and [e["kind"] for e in log] == ["reseed", "load", "reseed"]
        assert set(log[0]["ids"]) & set(log[1]["ids"]) and set(log[1]["ids"]) & set(log[2]["ids"])
        assert len(m["snaps"]) == 2          # (each save right behind a reseed)
    if "refrozen" in sc.claims:
        at = sc.info["refrozen_at"]
        assert not sc.auto_reset and done[at].all() and done[20].all() and [e[0] for e in sc.events][-2:] == ["reset", "steps"]
        assert not done[at + 1].all()          # (the reset() behind it: live again)
        first = next(e for e in log if e["kind"] == "reseed")
        assert (done[first["at"], first["ids"]] == 0).mean() > 0.5          # live again ...
        unl = np.setdiff1d(np.arange(n), sorted(listed))
        assert np.array_equal(m["steps"]["image"][at][unl], m["steps"]["image"][20][unl])
        assert m["starts"] == 2 * n + sum(len(e["ids"]) for e in log if e["kind"] == "reseed")
    if name == "bot":
        assert len(m["bot"]["action"]) == m["T"] and (m["bot"]["done"] != 0).any()


def test_every_claim_is_made_somewhere():
    claims = set()
    for c in su.COMMITTED:
        claims |= su.scenario(*c).claims
    assert {"two_episodes", "positions", "every_tick", "time_limit", "fan3", "edges", "majority", "one_window", "refrozen", "every_env"} <= claims


def test_token_rows_spell_the_missions():
    m = su.ScenarioModel("BossLevel", np.arange(40) + 7900)
    assert [detokenize(r) for r in m.tokens()] == m.missions()
