"""The scripts of tests/test_gpu_state_ranges.py -- bbai_export_state / bbai_import_state / bbai_get_programs on env ranges -- built on the host
model alone (scenario_util.ScenarioModel: no GPU), so that what they claim to reach is checked without a GPU (tests/test_scenario_host.py) and
the device tests only compare.  BBAI_LOOKAHEAD = 4 (scenario_util.B): an event in front of step s stands in front of window position (s + 1) % 4."""
import functools

import numpy as np

import scenario_util as su

N = 192
B = su.B
RANGES = [(0, 192), (0, 1), (191, 1), (63, 2), (64, 64), (1, 190), (130, 62), (0, 0), (192, 0)]
DONOR_SEED, RECIPIENT_SEED = 515100, 626200
DONOR_STEPS, AFTER = 20, 30
RESETS = 0.08          # scenario_util's rate of action 7 (BBAI_ACTION_RESET_ENV) per env and step


def seeds(base, n=N):
    return np.arange(n, dtype=np.uint64) + np.uint64(base)


def stepped_model(level, base, acts, done_actions=False, enum_done=False, n=N):
    m = su.ScenarioModel(level, seeds(base, n), done_actions=done_actions, enum_done=enum_done)
    for a in acts:
        m.step(a)
    return m


def state_rows(m, src=None):
    src = np.arange(m.n) if src is None else np.asarray(src, np.int64)
    return {"rec": m.hb.rec[src].copy(), "hot": m.hb.hot[src].copy(), "stale": m.hb.stale[src].copy()}


def donor_acts(n=N):
    return su._acts(DONOR_STEPS, n, 41, 0.0)


@functools.lru_cache(maxsize=None)
def donor(level, done_actions=False, enum_done=False):
    """The donor of the import tests: another seed, 20 random steps (auto-resetting).  Never written to."""
    return stepped_model(level, DONOR_SEED, donor_acts(), done_actions, enum_done)


def donor_sources(count, repeat=False, seed=43):
    """Which donor row goes into env first + k: `count` different rows in no order; repeat: row 5 seven times among them."""
    src = np.random.RandomState(seed).permutation(N)[:count].astype(np.int64)
    if repeat:
        assert count >= 16
        src[[0, 3, 4, 9, 10, 11, count - 1]] = 5
    return src


def import_script(level, first, count, pos, done_actions=False, enum_done=False, repeat=False):
    """3 + pos steps, the import of `count` donor rows into [first, first + count) in front of window position `pos`, 30 steps: random actions
    with reset commands.  -> (events, sources)"""
    pre = B - 1 + pos
    assert (pre + 1) % B == pos
    acts = su._acts(pre + AFTER, N, 50 + pos, RESETS)
    src = donor_sources(count, repeat)
    rows = state_rows(donor(level, done_actions, enum_done), src)
    return su._cut(acts, [0, pre]) + [("import", rows, first)] + su._cut(acts, [pre, pre + AFTER]), src


@functools.lru_cache(maxsize=None)
def import_run(level, first, count, pos, done_actions=False, enum_done=False, repeat=False):
    """The host model's outputs of import_script, its final state, and how many imported envs started a new episode behind the import."""
    ev, src = import_script(level, first, count, pos, done_actions, enum_done, repeat)
    m = su.ScenarioModel(level, seeds(RECIPIENT_SEED), done_actions=done_actions, enum_done=enum_done)
    out = m.run(ev)
    pre = B - 1 + pos
    restarted = (out["steps"]["done"][pre:, first:first + count] != 0).any(axis=0)
    return {"events": ev, "src": src, "model": out, "final": state_rows(m), "restarted": restarted, "pre": pre}


def twin_script(events):
    return [e for e in events if e[0] != "import"]


# ---- hot / stale-only imports (test 3) -------------------------------------------------------------------------------------------------------
POSE_FIRST, POSE_COUNT = 63, 66


def _turned(hot, k0=0):
    hot = hot.copy()
    hot[:, 2] = (hot[:, 2] + 1 + (np.arange(len(hot)) + k0) % 3) % 4          # Hot.dir: every env turns, by one, two or three quarters
    return hot


@functools.lru_cache(maxsize=None)
def pose_run(level):
    """Imports without records (rec NULL).  The rows are the recipient's OWN hot states and stale sets at that step -- the model's, which the
    device holds too: every step in front of the import is compared -- with nothing but Hot.dir changed, and every direction is a valid pose
    wherever an agent stands: so each pose is valid for the record it meets.  A hot-only import of envs 63 .. 128 in front of window position 1,
    a hot + stale import of every env in front of position 3, a stale-only import of envs 0 .. 63 in front of position 0; 30 steps behind."""
    marks = [0, B, B + 2, B + 3, B + 3 + AFTER]
    acts = su._acts(marks[-1], N, 70, RESETS)
    m = su.ScenarioModel(level, seeds(RECIPIENT_SEED + 2000))
    ev = []
    for j, (a, b) in enumerate(zip(marks, marks[1:])):
        ev += su._cut(acts, [a, b])
        for t in range(a, b):
            m.step(acts[t])
        if j == 0:
            e = ("import", {"rec": None, "hot": _turned(m.hb.hot[POSE_FIRST:POSE_FIRST + POSE_COUNT]), "stale": None}, POSE_FIRST)
        elif j == 1:
            e = ("import", {"rec": None, "hot": _turned(m.hb.hot, 1), "stale": m.hb.stale.copy()}, 0)
        elif j == 2:
            e = ("import", {"rec": None, "hot": None, "stale": m.hb.stale[:64].copy()}, 0)
        else:
            break
        m.import_state(e[1], e[2])
        ev.append(e)
    assert [(e[0] == "import") for e in ev].count(True) == 3
    r = su.ScenarioModel(level, seeds(RECIPIENT_SEED + 2000))
    out = r.run(ev)
    return {"events": ev, "model": out, "final": state_rows(r)}


# ---- done-action mode (test 4) ------------------------------------------------------------------------------------------------------------------
DONE_FIRST, DONE_COUNT = 60, 40


@functools.lru_cache(maxsize=None)
def done_case(enum_done=False):
    """GoToLocal under BABYAI_DONE_ACTIONS.  The donor steps with the six other actions until, from step 20 on, some live env stands in front of
    its target (lastStepMatch set); those envs' rows lead the 40 that go into envs 60 .. 99, in front of window position 2.  The first action
    behind the import is `done` for the whole range: it pays the donor's own envs and must pay nothing in the recipient, whose bytes are clear."""
    pre_d = su._acts(45, N, 4, 0.0) % 6
    d = su.ScenarioModel("GoToLocal", seeds(DONOR_SEED + 3000), done_actions=True, enum_done=enum_done)
    matched, steps = None, 0
    for t in range(45):
        d.step(pre_d[t])
        steps = t + 1
        matched = np.nonzero(d.hb.lsm != 0)[0]
        if t >= 19 and len(matched):
            break
    lsm = (d.hb.lsm != 0).astype(np.uint8)
    rest = [i for i in np.random.RandomState(81).permutation(N) if i not in set(matched.tolist())]
    src = np.array(matched.tolist() + rest, dtype=np.int64)[:DONE_COUNT]
    is_matched = np.isin(src, matched)
    rows = state_rows(d, src)
    d.step(np.full(N, 6, np.uint8))                      # the donor itself: `done` right behind the matching step
    paid = d.hb.reward64[matched].copy()
    pre = B - 1 + 2
    acts = su._acts(pre + AFTER, N, 82, 0.0) % 6
    acts[pre, DONE_FIRST:DONE_FIRST + DONE_COUNT] = 6
    acts[pre + 7] = 6
    ev = su._cut(acts, [0, pre]) + [("import", rows, DONE_FIRST)] + su._cut(acts, [pre, pre + AFTER])
    r = su.ScenarioModel("GoToLocal", seeds(RECIPIENT_SEED + 3000), done_actions=True, enum_done=enum_done)
    out = r.run(ev)
    return {"events": ev, "model": out, "final": state_rows(r), "donor_acts": pre_d[:steps], "donor_lsm": lsm, "src": src, "is_matched": is_matched,
            "donor_paid": paid, "pre": pre}


# ---- a fresh expert (test 7) ---------------------------------------------------------------------------------------------------------------
BOT_LEVEL, BOT_FIRST, BOT_COUNT, BOT_STEPS = "BossLevel", 70, 37, 10


@functools.lru_cache(maxsize=None)
def expert_case(level=BOT_LEVEL):
    """The recipient runs the expert for 10 steps on every env (a bot that gave up: the reset command, which ends the episode), the donor 10
    random steps; 37 donor rows go into envs 70 .. 106.  -> the decisions behind the import of the whole batch (model: a fresh Bot in the range, the
    old plans elsewhere), the same for a twin that did not import, and the colliding pairs: the row's Hot.step is 10 -- what the env's old
    plan expects -- and the env's own episode did not end in its 10 expert steps, so a plan that survived the import would have been continued."""
    r = su.ScenarioModel(level, seeds(RECIPIENT_SEED + 1000))
    ended = np.zeros(N, bool)
    acts = []
    for t in range(BOT_STEPS):
        act, _ = r.bot_decide()                         # (RESET_ENV where the bot gave up)
        r.step(act)
        ended |= r.hb.done != 0
        acts.append(act)
    d = stepped_model(level, DONOR_SEED + 1000, su._acts(BOT_STEPS, N, 61, 0.0))
    src = donor_sources(BOT_COUNT, seed=62)
    rows = state_rows(d, src)
    row_step = rows["hot"][:, 4].astype(np.int32) | rows["hot"][:, 5].astype(np.int32) << 8
    own = r.hb.step_count[BOT_FIRST:BOT_FIRST + BOT_COUNT]
    colliding = (row_step == BOT_STEPS) & ~ended[BOT_FIRST:BOT_FIRST + BOT_COUNT] & (own == BOT_STEPS)
    twin_states = r._bot_states.copy()
    twin = su.ScenarioModel(level, seeds(RECIPIENT_SEED + 1000))
    for k in ("rec", "hot", "stale", "mt", "mti"):
        getattr(twin.hb, k)[:] = getattr(r.hb, k)
    twin._bot_states, twin._bot_fresh = twin_states, r._bot_fresh.copy()
    r.import_state(rows, BOT_FIRST)
    want, gave = r.bot_decide()
    want_twin, gave_twin = twin.bot_decide()
    to255 = lambda a, g: np.where(g != 0, 255, a).astype(np.uint8)
    return {"rows": rows, "src": src, "want": to255(want, gave), "want_twin": to255(want_twin, gave_twin), "colliding": colliding,
            "expert_acts": np.stack(acts), "donor_acts": su._acts(BOT_STEPS, N, 61, 0.0)}
