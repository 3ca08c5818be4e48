"""Scripted runs of a batch -- steps with bbai_reseed / bbai_save_state / bbai_load_state in between -- on the host build (ScenarioModel, on
hostsim_util.HostBatch: no GPU) and on a BatchedBabyAIEnv under each step entry (run_device), with the same output arrays from both.

A script is a list of events:
    ("steps", acts uint8[T, n])            T steps of every env (7 = BBAI_ACTION_RESET_ENV)
    ("bot", T)                             T expert decisions + auto-reset steps (bbai_bot_rollout)
    ("reseed", ids, seeds)                 env.seed(s); env.reset() for the listed envs (ids None: every env); ids outside [0, n) are skipped
    ("reset",)                             reset() of the whole batch: every env's next level
    ("save", ids)                          snapshot of the listed envs; its index = the number of saves before it
    ("load", snap_index, ids, rows)        snapshot rows `rows` into envs `ids`
    ("import", donor_rows, first)          bbai_import_state: donor_rows = {"rec" uint8[count, rec_bytes] or None, "hot" uint8[count, 16] or None,
                                           "stale" uint64[count] or None} (export_state's arrays) into envs first .. first + count - 1

What a run returns (model: numpy; device: numpy after one copy at the end), `n` envs wide, never only the listed ones:
    "steps"   image [T, n, 7, 7, 3], direction [T, n], reward64 [T, n], reward [T, n], done [T, n], tokens [T, n, 72] after every step
    "bot"     image / direction / tokens the expert decided on, action, gave_up, reward, done, per bbai_bot_rollout step
    "calls"   per reseed / load / reset: image [n, 7, 7, 3], direction [n], tokens [n, 72] as the call leaves them
    "imports" per import: tokens [n, 72] as the call leaves them (an import writes no observation)
    "snaps"   per save: rec, hot, stale rows
    "starts"  episode starts: the reset, every reseeded env, every finished env of an auto-resetting step (bbai_reset_count)

The committed scenarios (BUILDERS, COMMITTED) are built for BBAI_LOOKAHEAD = 4: reset() is consume-tick 0 and every auto-resetting step one more, so
an event in front of step s stands in front of window position (s + 1) % 4.  tests/test_scenario_host.py pins the model to independent
references and asserts on the model alone what each scenario claims to reach."""
import collections
import ctypes
import functools

import numpy as np

from babyai_amd import missions
from babyai_amd.levels import make_cfg
from hostsim_util import HostBatch, lib

B = 4
RESET_ENV = 7
TOK_MAX = 72
OUT_KEYS = ("image", "direction", "reward64", "reward", "done")
BOT_KEYS = ("image", "direction", "tokens", "action", "gave_up", "reward", "done")
DEAD_CAPACITY = 2          # babyai_amd/csrc/bbai_bot.hpp: a fixed-size structure of the port overflowed (bbai_bot_stats counts these apart)


# ---- the host model ------------------------------------------------------------------------------------------------------------------------
class ScenarioModel(object):
    """n envs of the host build behind reset(), with the two calls modelled on HostBatch's arrays."""

    def __init__(self, level, seeds, auto_reset=True, done_actions=False, enum_done=False):
        self.level, self.cfg = level, make_cfg(level)
        self.L = lib()
        self.auto_reset = bool(auto_reset)
        self.hb = HostBatch(self.cfg, seeds, auto_reset=auto_reset, done_actions=done_actions, enum_done=enum_done)
        self.n = self.hb.n
        self.hb.reset()
        self.starts = self.n
        self.snaps = []
        self._tok = {}
        self._bot_states = None
        self._bot_fresh = np.ones(self.n, bool)
        self._own14 = {}            # env -> its level stream's own Hot.last_locked byte while its hot state shows a loaded row's (_take_hot)
        self.bot_stats = {"gave_up": 0, "capacity": 0}

    # Hot byte 14 (last_locked: LevelGen.locked_room, which survives episodes and feeds the next level's rand_obj) is state of the env's LEVEL
    # STREAM, like mt / mti: the engine generates from the ring's previous entry, never from the live hot state, so a loaded or imported env
    # goes on with its own.  Its live hot state SHOWS the loaded row's byte until the env's next episode starts, and so does hb.hot here; the
    # host build generates from hb.hot[i, 14] in place, so the env's own byte is kept apart and put back around everything that may generate.
    def _take_hot(self, i, row):
        self._own14.setdefault(i, self.hb.hot[i, 14])
        self.hb.hot[i, :15] = row[:15]          # (byte 15: the env's place in its own ring; mt / mti stay: its own next level)

    def _own_streams(self):
        """Before a call that may generate: every env's own byte 14 back in place.  -> what the hot states showed, for _shown_again."""
        shown = {i: self.hb.hot[i, 14] for i in self._own14}
        for i, b in self._own14.items():
            self.hb.hot[i, 14] = b
        return shown

    def _shown_again(self, shown, started):
        for i, b in shown.items():
            if started[i]:
                del self._own14[i]              # (the new episode's hot state came from the env's own stream)
            else:
                self.hb.hot[i, 14] = b

    # -- the calls
    def reseed(self, ids, seeds):
        hb = self.hb
        ids = np.arange(self.n) if ids is None else ids
        for i, s in zip(np.asarray(ids, np.int64).tolist(), np.asarray(seeds, np.uint64).tolist()):
            if not 0 <= i < self.n:
                continue
            one = HostBatch(self.cfg, [s])
            one.reset()
            for k in ("mt", "mti", "rec", "hot", "stale", "image", "direction"):
                getattr(hb, k)[i] = getattr(one, k)[0]
            hb.hot[i, 13] = 0           # (frozen)
            self._own14.pop(i, None)
            self._bot_fresh[i] = True
            self.starts += 1

    def reset(self):
        self._shown_again(self._own_streams(), np.ones(self.n, bool))
        self.hb.reset()
        self._bot_fresh[:] = True
        self.starts += self.n

    def save(self, ids):
        hb = self.hb
        ids = np.asarray(ids, np.int64)
        snap = {"rec": np.zeros((len(ids), self.cfg.rec_bytes), np.uint8), "hot": np.zeros((len(ids), 16), np.uint8), "stale": np.zeros(len(ids), np.uint64)}
        for k, i in enumerate(ids.tolist()):
            if 0 <= i < self.n:
                snap["rec"][k], snap["hot"][k], snap["stale"][k] = hb.rec[i], hb.hot[i], hb.stale[i]
        self.snaps.append(snap)
        return snap

    def load(self, snap, ids, rows):
        hb = self.hb
        for i, r in zip(np.asarray(ids, np.int64).tolist(), np.asarray(rows, np.int64).tolist()):
            if not (0 <= i < self.n and 0 <= r < len(snap["stale"])):
                continue
            hb.rec[i], hb.stale[i] = snap["rec"][r], snap["stale"][r]
            self._take_hot(i, snap["hot"][r])
            self.L.hs_observe(ctypes.byref(self.cfg), hb.rec[i].ctypes.data, hb.hot[i].ctypes.data, hb.image[i].ctypes.data)
            hb.direction[i] = hb.hot[i, 2]
            self._bot_fresh[i] = True

    def import_state(self, rows, first):
        """bbai_import_state(first, count, rec, hot, stale): load() on ids first .. first + count - 1 without the observation -- image and
        direction keep what the last step wrote.  With records the env's next expert decision starts a fresh Bot and its token row follows
        (tokens() reads the records); a hot- / stale-only import (rec None) moves neither.  Every import clears the done-action byte
        (lastStepMatch is no part of the exported state); the env keeps mt / mti: its own level stream."""
        hb = self.hb
        rec, hot, stale = rows.get("rec"), rows.get("hot"), rows.get("stale")
        count = len(next(x for x in (rec, hot, stale) if x is not None))
        assert first >= 0 and first + count <= self.n and all(x is None or len(x) == count for x in (rec, hot, stale))
        for k in range(count):
            i = first + k
            if rec is not None:
                hb.rec[i] = rec[k]
                self._bot_fresh[i] = True
            if hot is not None:
                self._take_hot(i, hot[k])
            if stale is not None:
                hb.stale[i] = stale[k]
            if hb.lsm is not None:
                hb.lsm[i] = 0

    # -- the steps
    def step(self, actions):
        hb = self.hb
        live = hb.hot[:, 13] == 0
        shown = self._own_streams()
        hb.step(actions)
        started = live & (hb.done != 0) & self.auto_reset
        self._shown_again(shown, started)
        self.starts += int(started.sum())

    def tokens(self):
        """The mission token rows uint8[n, 72] of the current records (missions.tokenize of prog_surface)."""
        c = self.cfg
        out = np.zeros((self.n, TOK_MAX), np.uint8)
        for i in range(self.n):
            prog = self.hb.rec[i, c.off_prog:c.off_prog + 112]
            key = prog[64:104].tobytes()
            row = self._tok.get(key)
            if row is None:
                ids = missions.tokenize(missions.prog_surface(prog))[:TOK_MAX]
                row = np.zeros(TOK_MAX, np.uint8)
                row[:len(ids)] = ids
                self._tok[key] = row
            out[i] = row
        return out

    def missions(self):
        c = self.cfg
        return [missions.prog_surface(self.hb.rec[i, c.off_prog:c.off_prog + 112]) for i in range(self.n)]

    def bot_decide(self, stack_cap=48):
        """One decision of the expert per env (hostsim_util.HostBot's call on this batch's rows): a fresh Bot at step_count == 0 and behind a
        reseed / load.  -> (actions with RESET_ENV where the bot gave up, gave_up)."""
        hb, L = self.hb, self.L
        if self._bot_states is None:
            self._bot_states = np.zeros((self.n, L.hs_bot_state_bytes(stack_cap)), np.uint8)
        act, gave = np.zeros(self.n, np.uint8), np.zeros(self.n, np.uint8)
        steps = hb.step_count
        for i in range(self.n):
            first = bool(self._bot_fresh[i]) or steps[i] == 0
            st = self._bot_states[i]
            a = L.hs_bot_decide(ctypes.byref(self.cfg), hb.rec[i].ctypes.data, hb.hot[i].ctypes.data, hb.stale[i:i + 1].ctypes.data, st.ctypes.data,
                                stack_cap, 1 if first else 0, -1)
            assert 0 <= a <= 255, a
            self._bot_fresh[i] = False
            if a == 255:
                gave[i] = 1
                self.bot_stats["capacity" if L.hs_bot_dead_reason(st.ctypes.data) == DEAD_CAPACITY else "gave_up"] += 1
                self._bot_fresh[i] = True          # (its RESET_ENV ends the episode: step_count 0 next, a fresh Bot either way)
                a = RESET_ENV
            act[i] = a
        return act, gave

    # -- a whole script
    def run(self, events):
        hb = self.hb
        steps = {k: [] for k in OUT_KEYS + ("tokens",)}
        bot = {k: [] for k in BOT_KEYS}
        calls, imports, log = [], [], []
        reset = {"image": hb.image.copy(), "direction": hb.direction.copy(), "tokens": self.tokens()}

        def emit():
            for k in OUT_KEYS:
                steps[k].append(getattr(hb, k).copy())
            steps["tokens"].append(self.tokens())

        for ev in events:
            at = len(steps["done"])
            if ev[0] == "steps":
                for a in ev[1]:
                    self.step(a)
                    emit()
            elif ev[0] == "bot":
                for _ in range(ev[1]):
                    bot["image"].append(hb.image.copy()); bot["direction"].append(hb.direction.copy()); bot["tokens"].append(self.tokens())
                    act, gave = self.bot_decide()
                    self.step(act)
                    bot["action"].append(act); bot["gave_up"].append(gave); bot["reward"].append(hb.reward); bot["done"].append(hb.done.copy())
                    emit()
            elif ev[0] == "reseed":
                self.reseed(ev[1], ev[2])
                ok = [int(i) for i in (range(self.n) if ev[1] is None else ev[1]) if 0 <= i < self.n]
                log.append({"kind": "reseed", "at": at, "ids": ok, "all": ev[1] is None})
            elif ev[0] == "reset":
                self.reset()
            elif ev[0] == "save":
                self.save(ev[1])
                continue
            elif ev[0] == "load":
                snap = self.snaps[ev[1]]
                ok = [(int(i), int(r)) for i, r in zip(ev[2], ev[3]) if 0 <= i < self.n and 0 <= r < len(snap["stale"])]
                hot = snap["hot"][[r for _, r in ok]].astype(np.int32)
                log.append({"kind": "load", "at": at, "ids": [i for i, _ in ok], "rows": [r for _, r in ok], "step_count": hot[:, 4] | hot[:, 5] << 8,
                            "max_steps": hot[:, 6] | hot[:, 7] << 8, "frozen": hot[:, 13]})
                self.load(snap, ev[2], ev[3])
            elif ev[0] == "import":
                self.import_state(ev[1], ev[2])
                count = len(next(x for x in ev[1].values() if x is not None))
                log.append({"kind": "import", "at": at, "ids": list(range(ev[2], ev[2] + count)), "rec": ev[1].get("rec") is not None})
                imports.append({"tokens": self.tokens()})
            else:
                raise ValueError(ev[0])
            if ev[0] in ("reseed", "load", "reset"):
                calls.append({"image": hb.image.copy(), "direction": hb.direction.copy(), "tokens": self.tokens()})
        T = len(steps["done"])
        shapes = {"image": (0, self.n, 7, 7, 3), "tokens": (0, self.n, TOK_MAX)}
        stack = lambda d: {k: np.stack(v) if v else np.zeros(shapes.get(k, (0, self.n)), np.uint8) for k, v in d.items()}
        return {"steps": stack(steps), "bot": stack(bot), "calls": calls, "imports": imports, "snaps": self.snaps, "starts": self.starts, "log": log, "reset": reset, "T": T,
                "bot_stats": dict(self.bot_stats)}


# ---- the committed scenarios ----------------------------------------------------------------------------------------------------------
def listed_ids(n, k, seed=3):
    """k envs that include 0 and n - 1 and both sides of every 64-env boundary, in no order (test_gpu_reseed._ids37's idea for any n)."""
    edge = [0, n - 1] + [b + d for b in range(64, n, 64) for d in (-1, 0) if 0 < b + d < n - 1]
    rng = np.random.RandomState(seed)
    rest = [i for i in rng.permutation(n) if i not in edge]
    ids = np.array(edge + rest[:k - len(edge)], dtype=np.int64)
    assert len(ids) == k and len(set(ids.tolist())) == k
    return rng.permutation(ids)


def new_seeds(k, base):
    return np.arange(k, dtype=np.uint64) * np.uint64(17) + np.uint64(base)


def _groups(n, sizes, seed):
    """Disjoint id groups of the given sizes (scaled down for a small batch) out of listed_ids."""
    scale = 1.0 if n >= 128 else 0.5
    sizes = [max(2, int(round(s * scale))) for s in sizes]
    ids = listed_ids(n, sum(sizes), seed)
    cuts = np.cumsum([0] + sizes)
    return [ids[a:b] for a, b in zip(cuts, cuts[1:])]


def _acts(T, n, seed, resets):
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 7, size=(T, n)).astype(np.uint8)
    if resets:
        a[rng.rand(T, n) < resets] = RESET_ENV
    return a


def _fan(rows, dst):
    """Snapshot rows for the envs `dst`: the first rows go into THREE envs each, the others into one."""
    out, r = [], 0
    while len(out) < len(dst):
        out += [rows[r % len(rows)]] * (3 if r < max(1, len(dst) // 6) else 1)
        r += 1
    return np.array(out[:len(dst)], dtype=np.int64)


def _cut(acts, marks):
    return [("steps", acts[a:b]) for a, b in zip(marks, marks[1:])]


def _main(level, n):
    """Reseeds in front of window positions 1, B - 1 and 0 -- the first env of the position-1 and position-0 groups then finishes on every tick the
    window has left (action 7: the latter consumes B + 1 slots in that window) --, a save and a load in mid-run, and, on GoToLocal, states saved one
    step from their time limit loaded into three envs each: they time out on the next tick and take their own rings' next levels."""
    T = 140
    resets = 0.0 if level == "GoToLocal" else 0.08
    a1, a2, a3, c, d, x, y = _groups(n, [6, 5, 6, 6, 12, 4, 12], 3)
    acts = _acts(T, n, 11, resets)
    acts[0:B - 1, a1[0]] = RESET_ENV
    acts[B - 1:2 * B - 1, a3[0]] = RESET_ENV
    acts[:63, x] &= 1                    # left / right only (63 steps without an end unless the agent turns to face its target)
    s0 = np.concatenate([a1, c])
    ev = [("reseed", a1, new_seeds(len(a1), 9000000))] + _cut(acts, [0, 2]) + [("reseed", a2, new_seeds(len(a2), 9100000))] + _cut(acts, [2, 3]) + \
         [("reseed", a3, new_seeds(len(a3), 9200000))] + _cut(acts, [3, 7]) + [("save", s0)] + _cut(acts, [7, 9]) + \
         [("load", 0, d, _fan(np.arange(len(s0)), d))] + _cut(acts, [9, 63]) + [("save", x), ("load", 1, y, np.repeat(np.arange(len(x)), 3)[:len(y)])] + \
         _cut(acts, [63, T])
    claims = {"two_episodes", "positions", "every_tick", "fan3", "edges", "majority"} | ({"time_limit"} if level == "GoToLocal" else set())
    return ev, claims, {"every_tick": [(int(a1[0]), 0, B - 1), (int(a3[0]), B - 1, 2 * B - 1)]}


def _mixed(level, n):
    """Both calls inside ONE window (steps 3 .. 6 = window positions 0 .. 3): reseed A, save A and C at once, load those rows into D -- which holds
    envs of A, reseeded in this window, and one row goes into three envs --, then reseed envs of D that were just loaded."""
    T = 140
    resets = 0.0 if level == "GoToLocal" else 0.08
    a, c, d = _groups(n, [10, 6, 12], 5)
    d = np.concatenate([a[1:3], d])
    acts = _acts(T, n, 12, resets)
    s0 = np.concatenate([a, c])
    e = np.array([d[0], d[3], d[len(d) - 1]], dtype=np.int64)
    ev = _cut(acts, [0, 3]) + [("reseed", a, new_seeds(len(a), 9300000)), ("save", s0)] + _cut(acts, [3, 4]) + [("load", 0, d, _fan(np.arange(len(s0)), d))] + \
        _cut(acts, [4, 5]) + [("reseed", e, new_seeds(len(e), 9400000)), ("save", e)] + _cut(acts, [5, T])
    return ev, {"two_episodes", "fan3", "edges", "majority", "one_window"}, {}


def _storm(level, n):
    """Eight envs on the batch's edges reseeded in front of window position 0 TWICE in consecutive windows while they finish on every tick of both
    (action 7: B + 1 slots consumed in each), the second time with a save and a load into them in front of the same tick; then EVERY env reseeded
    (ids None) in mid-window; then a reseed and a load in front of the next window's positions 0 and 1."""
    T = 140
    resets = 0.0 if level == "GoToLocal" else 0.08
    s = listed_ids(n, 8, 13)
    acts = _acts(T, n, 15, resets)
    acts[B - 1:3 * B - 1, s] = RESET_ENV
    ev = _cut(acts, [0, 3]) + [("reseed", s, new_seeds(8, 9900000))] + _cut(acts, [3, 7]) + \
        [("reseed", s, new_seeds(8, 9910000)), ("save", s), ("load", 0, s[1:4], np.zeros(3, np.int64))] + _cut(acts, [7, 9]) + \
        [("reseed", None, new_seeds(n, 9920000))] + _cut(acts, [9, 11]) + [("reseed", s[:4], new_seeds(4, 9930000))] + _cut(acts, [11, 12]) + \
        [("load", 0, s[4:], np.arange(4, 8))] + _cut(acts, [12, T])
    return ev, {"two_episodes", "every_tick", "fan3", "edges", "every_env"}, {"every_tick": [(int(i), B - 1, 2 * B - 1) for i in s] + [(int(i), 2 * B - 1, 3 * B - 1) for i in s]}


def _frozen(level, n):
    """auto_reset=False: 20 steps, a reset command for everyone (the whole batch is frozen), then frozen envs reseeded live again, their states
    loaded into other frozen envs, a second reseed while the first group runs, 70 steps in one piece, behind which everything froze again -- and a
    reset() of the whole batch (the reseeded envs take level 1 of their new streams, the others their next) with 20 steps behind it."""
    T = 96
    resets = 0.0 if level == "GoToLocal" else 0.08
    a, d, e = _groups(n, [14, 12, 8], 7)
    acts = _acts(T, n, 13, resets)
    acts[20] = RESET_ENV
    acts[21:24, a] %= 3                  # (turns and moves: the states saved behind them are live ones)
    ev = _cut(acts, [0, 21]) + [("reseed", a, new_seeds(len(a), 9500000))] + _cut(acts, [21, 24]) + [("save", a), ("load", 0, d, _fan(np.arange(len(a)), d))] + \
        _cut(acts, [24, 26]) + [("reseed", e, new_seeds(len(e), 9600000))] + _cut(acts, [26, T]) + [("reset",)] + [("steps", _acts(20, n, 14, resets))]
    return ev, {"fan3", "edges", "majority", "refrozen"}, {"refrozen_at": T - 1}


def _bot(level, n):
    """The expert drives (bbai_bot_rollout chunks): reseed in front of window position 0, save, load with one row into three envs, reseed of loaded envs."""
    rest = 60 if level == "GoToLocal" else 130
    a, c, d = _groups(n, [12, 6, 18], 9)
    s0 = np.concatenate([a, c])
    ev = [("bot", 3), ("reseed", a, new_seeds(len(a), 9700000)), ("bot", 4), ("save", s0), ("bot", 2), ("load", 0, d, _fan(np.arange(len(s0)), d)), ("bot", 1),
          ("reseed", d[:2], new_seeds(2, 9800000)), ("bot", rest)]
    return ev, {"fan3", "edges", "majority"} | ({"two_episodes"} if level == "GoToLocal" else {"one_episode"}), {}


Scenario = collections.namedtuple("Scenario", "name level n auto_reset events claims info seeds")
BUILDERS = {"main": (_main, True), "mixed": (_mixed, True), "storm": (_storm, True), "frozen": (_frozen, False), "bot": (_bot, True)}
SEED_BASE = 424200


@functools.lru_cache(maxsize=None)
def scenario(name, level, n):
    build, auto = BUILDERS[name]
    events, claims, info = build(level, n)
    return Scenario(name, level, n, auto, events, frozenset(claims), info, np.arange(n, dtype=np.uint64) + np.uint64(SEED_BASE))


@functools.lru_cache(maxsize=None)
def model_run(name, level, n):
    """The host model's outputs of a committed scenario: computed once per process, shared by every test, never written to."""
    sc = scenario(name, level, n)
    return ScenarioModel(level, sc.seeds, auto_reset=sc.auto_reset).run(sc.events)


# ---- the device side ------------------------------------------------------------------------------------------------------------------
# (scenario, level, n) of every run tests/test_gpu_reseed_snapshot_entries.py makes: tests/test_scenario_host.py checks each one's claims on the model
COMMITTED = [("main", lv, n) for lv, n in (("GoToLocal", 192), ("GoToLocal", 65), ("BossLevel", 192), ("PutNextS5N2Carrying", 192))] + \
    [("mixed", "GoToLocal", 192), ("mixed", "BossLevel", 192), ("storm", "GoToLocal", 192), ("storm", "BossLevel", 192), ("frozen", "GoToLocal", 192), ("frozen", "GoToLocal", 65), ("frozen", "BossLevel", 192),
     ("bot", "GoToLocal", 65), ("bot", "BossLevel", 65)]
ENTRIES = ("step", "ticks", "ticks_frozen", "rollout_tokens", "step_tapped", "dstore", "dstore_split", "dstore_abi", "bot_rollout")


def _abi_reseed(env, ids, seeds):
    from babyai_amd.engine import _check
    k, seeds_t = env._reseed_args(ids, seeds)
    _, ids_ptr, ids_t = env._ids(ids)
    env._hold["reseed"] = (ids_t, seeds_t)
    _check(env.lib, env.lib.bbai_reseed(env.handle, ids_ptr, seeds_t.data_ptr(), k, env.image.data_ptr(), env.direction.data_ptr(), env._stream()), "bbai_reseed")


def _abi_load(env, snap, ids, rows):
    from babyai_amd.engine import _check
    k, ids_ptr, ids_t = env._ids(ids)
    _, rows_ptr, rows_t = env._ids(rows)
    env._hold["load_state"] = (snap, ids_t, rows_t)
    _check(env.lib, env.lib.bbai_load_state(env.handle, ids_ptr, rows_ptr, k, len(snap), snap.rec.data_ptr(), snap.hot.data_ptr(), snap.stale.data_ptr(),
                                             snap.lsm.data_ptr(), env.image.data_ptr(), env.direction.data_ptr(), env._stream()), "bbai_load_state")


def abi_import(env, rows, first):
    """bbai_import_state through the library handle: env.import_state() takes all three arrays, the entry point takes NULL for any of them
    (rec NULL = a hot- / stale-only import).  The host arrays are read before the call returns."""
    from babyai_amd.engine import _check
    rec, hot, stale = rows.get("rec"), rows.get("hot"), rows.get("stale")
    count = len(next(x for x in (rec, hot, stale) if x is not None))
    rec = None if rec is None else np.ascontiguousarray(rec, dtype=np.uint8).reshape(count, env.cfg.rec_bytes)
    hot = None if hot is None else np.ascontiguousarray(hot, dtype=np.uint8).reshape(count, 16)
    stale = None if stale is None else np.ascontiguousarray(stale, dtype=np.uint64).reshape(count)
    ptr = lambda a: None if a is None else a.ctypes.data
    _check(env.lib, env.lib.bbai_import_state(env.handle, int(first), count, ptr(rec), ptr(hot), ptr(stale)), "bbai_import_state")


def run_device(env, events, entry, tap_ids=None, after=None):
    """The script on `env` (reset() behind it already) under step entry `entry`; the model's arrays back, as numpy.  `after(kind, index)` is called
    behind every step ("step", step index) and call ("call", call index) of the per-step entries, for checks of buffers the result does not carry
    (pixels).  The per-step rows of the rollout entries come from their tap logs: no "reward" there; "finals" holds every output buffer as each
    rollout call left it, keyed by the index of its last step.  step_tapped: "tapped" holds the listed envs' log rows per step."""
    import torch
    n, dev = env.num_envs, env.device
    tokens_on = getattr(env, "instr", None) is not None
    abi = entry == "dstore_abi"
    keys = OUT_KEYS if entry in ("step", "step_tapped", "dstore", "dstore_split", "dstore_abi", "bot_rollout") else ("image", "direction", "reward64", "done")
    steps = {k: [] for k in keys + (("tokens",) if tokens_on else ())}
    bot = {k: [] for k in BOT_KEYS}
    tapped = {k: [] for k in ("image", "direction", "reward64", "done")}
    calls, imports, snaps, finals = [], [], [], {}
    count = 0

    def emit():
        for k in keys:
            steps[k].append(getattr(env, k).clone())
        if tokens_on:
            steps["tokens"].append(env.instr.clone())

    def new_log(T, p):
        return {"image": torch.zeros((T, p, 7, 7, 3), dtype=torch.uint8, device=dev), "direction": torch.zeros((T, p), dtype=torch.uint8, device=dev),
                "reward64": torch.zeros((T, p), dtype=torch.float64, device=dev), "done": torch.zeros((T, p), dtype=torch.uint8, device=dev)}

    if entry in ("ticks", "ticks_frozen"):
        env.set_step_tap(list(range(n)))
    elif entry == "step_tapped":
        env.set_step_tap([int(i) for i in tap_ids])
    elif entry == "rollout_tokens":
        order = torch.as_tensor(np.random.RandomState(1).permutation(n).astype(np.int64), device=dev)       # log row k = env order[k]
    for ev in events:
        if ev[0] == "steps":
            acts = torch.as_tensor(np.ascontiguousarray(ev[1]), device=dev)
            T = int(acts.shape[0])
            if entry in ("step", "dstore", "dstore_split", "dstore_abi"):
                for t in range(T):
                    env.step(acts[t])
                    emit()
                    if after:
                        after("step", count + t)
            elif entry == "step_tapped":
                for t in range(T):
                    log = new_log(1, len(tap_ids))
                    env.step_tapped(acts[t], log["image"][0], log["direction"][0], log["reward64"][0], log["done"][0])
                    emit()
                    for k in tapped:
                        tapped[k].append(log[k][0])
            elif entry in ("ticks", "ticks_frozen", "rollout_tokens"):
                log = new_log(T, n)
                if entry == "rollout_tokens":
                    log["ids"] = order
                env.rollout(acts, tap=log, step_tap=entry != "rollout_tokens")
                for t in range(T):
                    for k in keys:
                        if entry == "rollout_tokens":
                            row = torch.empty_like(log[k][t])
                            row[order] = log[k][t]
                            steps[k].append(row)
                        else:
                            steps[k].append(log[k][t])
                    if tokens_on:          # (the token rows are not part of a tap log: the last step's are checked)
                        steps["tokens"].append(env.instr.clone() if t == T - 1 else None)
                finals[count + T - 1] = {k: getattr(env, k).clone() for k in OUT_KEYS}
            else:
                raise ValueError("entry %s takes no ('steps', ...) event" % entry)
            count += T
        elif ev[0] == "bot":
            r = env.bot_rollout(ev[1], tokens=True)
            for k in BOT_KEYS:
                bot[k].append(r[k])
            count += ev[1]
        elif ev[0] == "save":
            snaps.append(env.save_state(ev[1]))
        elif ev[0] == "import":
            abi_import(env, ev[1], ev[2])
            imports.append({"tokens": env.instr.clone() if tokens_on else None})
            if after:
                after("import", len(imports) - 1)
        else:
            if ev[0] == "reseed":
                ids = None if ev[1] is None else np.asarray(ev[1], np.int64)
                if abi:
                    _abi_reseed(env, ids, ev[2])
                else:
                    env.reseed(ids, ev[2])
            elif ev[0] == "reset":
                env.reset()
            else:
                ids, rows = np.asarray(ev[2], np.int64), np.asarray(ev[3], np.int64)
                if abi:
                    _abi_load(env, snaps[ev[1]], torch.as_tensor(ids, device=dev), torch.as_tensor(rows, device=dev))
                else:
                    env.load_state(snaps[ev[1]], ids=ids, rows=torch.as_tensor(rows, device=dev))
            calls.append({"image": env.image.clone(), "direction": env.direction.clone(), "tokens": env.instr.clone() if tokens_on else None})
            if after:
                after("call", len(calls) - 1)
    torch.cuda.current_stream(dev).synchronize()
    cpu = lambda t: None if t is None else t.cpu().numpy()
    out = {"steps": {k: [cpu(x) for x in v] for k, v in steps.items()}, "calls": [{k: cpu(v) for k, v in c.items()} for c in calls],
           "imports": [{k: cpu(v) for k, v in c.items()} for c in imports],
           "bot": {k: np.concatenate([cpu(x) for x in v]) if v else None for k, v in bot.items()},
           "snaps": [{"rec": cpu(s.rec), "hot": cpu(s.hot), "stale": cpu(s.stale).view(np.uint64)} for s in snaps],
           "finals": {t: {k: cpu(v) for k, v in f.items()} for t, f in finals.items()}, "tapped": {k: [cpu(x) for x in v] for k, v in tapped.items()}, "T": count}
    return out


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32) if a.dtype == np.float32 else a


def _same(what, got, want):
    got, want = _bits(got), _bits(want)
    if got.shape != want.shape or not np.array_equal(got, want):
        bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0] if got.shape == want.shape else "shapes %s / %s" % (got.shape, want.shape)
        raise AssertionError("%s differs from the host model in envs %s" % (what, bad[:12].tolist() if not isinstance(bad, str) else bad))


def assert_equals_model(got, want, tap_ids=None):
    """Every byte the device run returned against the host model's: all n envs of every step and call, reward64 and reward by bit pattern."""
    assert got["T"] == want["T"], (got["T"], want["T"])
    for k, rows in got["steps"].items():
        assert not rows or len(rows) == want["T"], (k, len(rows))
        for t, row in enumerate(rows):
            if row is not None:
                _same("step %d %s" % (t, k), row, want["steps"][k][t])
    for t, f in got["finals"].items():
        for k, v in f.items():
            _same("buffer %s behind the rollout call that ends with step %d" % (k, t), v, want["steps"][k][t])
    for k, rows in got["tapped"].items():
        for t, row in enumerate(rows):
            _same("step %d tap row %s" % (t, k), row, want["steps"][k][t][np.asarray(tap_ids)])
    assert len(got["calls"]) == len(want["calls"])
    for j, (c, w) in enumerate(zip(got["calls"], want["calls"])):
        for k in ("image", "direction", "tokens"):
            if c[k] is not None:
                _same("call %d %s" % (j, k), c[k], w[k])
    assert len(got.get("imports", ())) == len(want.get("imports", ()))
    for j, (c, w) in enumerate(zip(got.get("imports", ()), want.get("imports", ()))):
        if c["tokens"] is not None:
            _same("import %d tokens" % j, c["tokens"], w["tokens"])
    assert len(got["snaps"]) == len(want["snaps"])
    for j, (s, w) in enumerate(zip(got["snaps"], want["snaps"])):
        _same("snapshot %d rec" % j, s["rec"], w["rec"])
        _same("snapshot %d hot bytes 0..14" % j, s["hot"][:, :15], w["hot"][:, :15])
        _same("snapshot %d stale" % j, s["stale"], w["stale"])
    for k, v in got["bot"].items():
        if v is not None:
            for t in range(len(v)):
                _same("bot_rollout step %d %s" % (t, k), v[t], want["bot"][k][t])
