"""Helpers of the tests of SHORT reseeds (include/bbai.h bbai_reseed, option "reseed_levels"): the host model with a
level budget per env that parks (ParkingModel, on scenario_util.ScenarioModel), the scripted runs with their depths, what lets
scenario_util.run_device pass those depths to a BatchedBabyAIEnv (WithLevels), the comparison that leaves a parked env's unspecified outputs
out, and the host build behind the two pool schedulers' env protocols with `levels` honoured (HostPoolLevels, HostEvalEnv).

A script is one of scenario_util's with a fourth element in its reseed events: ("reseed", ids, seeds, levels).  The scenarios are built for
BBAI_LOOKAHEAD = 4 (ring depth 8): reset() is consume-tick 0, so an event in front of step s stands in front of window position (s + 1) % 4."""
import collections
import ctypes
import functools

import numpy as np

import scenario_util as su
from scenario_util import B, RESET_ENV, ScenarioModel
from seed_demos_util import HostPool

RING = 2 * B                 # D - inplace at BBAI_LOOKAHEAD = 4: a depth of 0 or >= RING is the whole ring
DEPTHS = (1, 2, 3, RING, RING + 5)
A_DONE = 6
FOREVER = 1 << 40
MASKED = ("image", "direction", "tokens")          # unspecified for a parked env


# ---- the host model ------------------------------------------------------------------------------------------------------------------------
class ParkingModel(ScenarioModel):
    """ScenarioModel + `levels_left` per env: a short reseed gives the env k levels; every move to a next level (an auto-reset, a reset())
    takes one; the move that takes the last one PARKS the env -- frozen, its reward and done as the last episode left them, the expert
    answering `done` -- until a reseed.  What the host build generated for the parked env meanwhile is the unspecified part."""

    def __init__(self, level, seeds, ring=RING, **kw):
        super().__init__(level, seeds, **kw)
        self.ring = int(ring)
        self.levels_left = np.full(self.n, FOREVER, np.int64)
        self.parked = np.zeros(self.n, bool)
        self.depths = collections.deque()       # run(): the depth of each reseed event, in order
        self.before, self.after, self.after_call = [], [], []       # parked masks: in front of / behind every step, behind every reseed / load / reset

    def _moved(self, moved):
        for i in np.flatnonzero(moved).tolist():
            if not self.parked[i] and self.levels_left[i] < FOREVER:
                self.levels_left[i] -= 1
                if self.levels_left[i] == 0:
                    self.parked[i] = True
        self.hb.hot[self.parked, 13] = 1

    def reseed(self, ids, seeds, levels=None):
        k = int(self.depths.popleft() if levels is None and self.depths else (levels or 0))
        super().reseed(ids, seeds)
        listed = np.arange(self.n) if ids is None else np.asarray(ids, np.int64)
        listed = listed[(listed >= 0) & (listed < self.n)]
        self.levels_left[listed] = k if 0 < k < self.ring else FOREVER
        self.parked[listed] = False
        self.after_call.append(self.parked.copy())

    def reset(self):
        super().reset()
        self._moved(np.ones(self.n, bool))
        self.after_call.append(self.parked.copy())

    def load(self, snap, ids, rows):
        super().load(snap, ids, rows)
        self.after_call.append(self.parked.copy())

    def step(self, actions):
        hb = self.hb
        self.before.append(self.parked.copy())
        live = hb.hot[:, 13] == 0
        super().step(actions)
        self._moved(live & (hb.done != 0) & self.auto_reset)
        self.after.append(self.parked.copy())

    def bot_decide(self, stack_cap=48):
        """ScenarioModel.bot_decide with k_bot's answer for a frozen env: `done`, gave_up = 0, the env's plan untouched."""
        hb, L = self.hb, self.L
        if self._bot_states is None:
            self._bot_states = np.zeros((self.n, L.hs_bot_state_bytes(stack_cap)), np.uint8)
        act, gave = np.zeros(self.n, np.uint8), np.zeros(self.n, np.uint8)
        steps = hb.step_count
        for i in range(self.n):
            if hb.hot[i, 13]:
                act[i] = A_DONE
                continue
            first = bool(self._bot_fresh[i]) or steps[i] == 0
            st = self._bot_states[i]
            a = L.hs_bot_decide(ctypes.byref(self.cfg), hb.rec[i].ctypes.data, hb.hot[i].ctypes.data, hb.stale[i:i + 1].ctypes.data, st.ctypes.data,
                                stack_cap, 1 if first else 0, -1)
            assert 0 <= a <= 255, a
            self._bot_fresh[i] = False
            if a == 255:
                gave[i] = 1
                self.bot_stats["capacity" if L.hs_bot_dead_reason(st.ctypes.data) == su.DEAD_CAPACITY else "gave_up"] += 1
                self._bot_fresh[i] = True
                a = RESET_ENV
            act[i] = a
        return act, gave

    def run(self, events):
        self.depths = collections.deque(int(ev[3]) if len(ev) > 3 else 0 for ev in events if ev[0] == "reseed")
        out = super().run(events)
        stack = lambda rows: np.stack(rows) if rows else np.zeros((0, self.n), bool)
        out["parked_before"], out["parked"], out["parked_calls"] = stack(self.before), stack(self.after), list(self.after_call)
        return out


# ---- the scripted runs --------------------------------------------------------------------------------------------------------------------
def _by_depth(n, seed):
    """The 37 listed envs (0, n - 1, both sides of every 64-env boundary among them) in five groups, one per depth of DEPTHS."""
    ids = su.listed_ids(n, 37, seed)
    cuts = np.cumsum([0, 9, 8, 8, 6, 6])
    return [ids[a:b] for a, b in zip(cuts, cuts[1:])]


def _short(level, n):
    """Auto-reset.  Every depth group is reseeded in three parts: in front of window position 0 (step 3), in mid-window (step 5) and in front
    of the window's last tick (step 6).  Behind its reseed a listed env ends an episode (action 7) on every third step -- the first of each
    group on EVERY step, so it spends its levels inside one window -- up to eight times: depth 1, 2 and 3 park behind one, two and three of
    them, depth RING (the whole ring) and RING + 5 never.  In front of step 26 -- more than two windows behind the last parking of the
    every-third-step envs -- parked envs of depth 1 come back through a reseed at depth 1 (and park again) and parked envs of depth 2
    through one at depth 0 (and never park again); the rest stay parked to the end."""
    T = 44
    resets = 0.0 if level in ("GoToLocal", "PutNextS5N2Carrying") else 0.08
    groups = _by_depth(n, 21)
    acts = su._acts(T, n, 31, resets)
    listed = np.concatenate(groups)
    acts[:, listed] = np.where(acts[:, listed] == RESET_ENV, 0, acts[:, listed])          # the listed envs end episodes where the script says
    at = {3: [], 5: [], 6: []}
    for g, k in zip(groups, DEPTHS):
        for part, s in zip(np.array_split(g, 3), (3, 5, 6)):
            at[s].append((part, k))
            for j, i in enumerate(part.tolist()):
                every = 1 if (j == 0 and s == 3) else 3
                ends = [s + every * (m + 1) - 1 for m in range(8) if s + every * (m + 1) - 1 < 25]
                acts[ends, i] = RESET_ENV
    ev, base = [], 7000000
    marks = [0, 3, 5, 6, 26, T]
    for a, b in zip(marks, marks[1:]):
        ev += su._cut(acts, [a, b])
        for part, k in at.get(b, []):
            base += 1000
            ev.append(("reseed", part, su.new_seeds(len(part), base), k))
        if b == 26:
            ev.append(("reseed", groups[0][:5], su.new_seeds(5, 7900000), 1))
            ev.append(("reseed", groups[1][:4], su.new_seeds(4, 7910000), 0))
            acts[[29, 33], groups[0][0]] = RESET_ENV          # (parks again at step 29; a parked env ignores the action of step 33)
            acts[[29, 33, 37], groups[1][0]] = RESET_ENV      # (depth 0: three more episodes and no parking)
    info = {"groups": groups, "again1": groups[0][:5], "again0": groups[1][:4], "again_at": 26,
            "one_window": [int(g[0]) for g in groups[:3]]}
    return ev, info


def _frozen(level, n):
    """auto_reset=False: 6 steps, the last one a reset command for everyone (the batch is frozen); group A reseeded at depth 1, group B at depth
    2, group C at depth 0 (live again); 3 steps that end with the three groups' episodes ended; ONE reset() of the whole batch -- A moves past
    its one level and parks, B and C take level 1 of their new streams, everyone else their next level --; 12 steps (three windows)."""
    resets = 0.0 if level in ("GoToLocal", "PutNextS5N2Carrying") else 0.08
    ids = su.listed_ids(n, 37, 23)
    a, b, c = ids[:13], ids[13:25], ids[25:]
    acts = su._acts(21, n, 33, resets)
    acts[5] = RESET_ENV
    acts[8, ids] = RESET_ENV
    ev = su._cut(acts, [0, 6]) + [("reseed", a, su.new_seeds(len(a), 7100000), 1), ("reseed", b, su.new_seeds(len(b), 7200000), 2),
                                 ("reseed", c, su.new_seeds(len(c), 7300000), 0)] + su._cut(acts, [6, 9]) + [("reset",)] + su._cut(acts, [9, 21])
    return ev, {"groups": [a, b, c], "reset_at": 9}


def _bot(level, n):
    """The expert drives (bbai_bot_rollout chunks): a third of the listed envs reseeded at depth 1, a third at depth 2, a third at depth RING + 5,
    in front of window position 0; GoToLocal episodes take the expert a handful of steps, so the first two thirds park inside the next chunk;
    then parked envs come back at depth 1 and at depth 0."""
    ids = su.listed_ids(n, 37, 25)
    a, b, c = ids[:13], ids[13:25], ids[25:]
    ev = [("bot", 3), ("reseed", a, su.new_seeds(len(a), 7400000), 1), ("reseed", b, su.new_seeds(len(b), 7500000), 2),
          ("reseed", c, su.new_seeds(len(c), 7600000), RING + 5), ("bot", 30), ("reseed", a[:6], su.new_seeds(6, 7700000), 1),
          ("reseed", b[:6], su.new_seeds(6, 7800000), 0), ("bot", 12)]
    return ev, {"groups": [a, b, c], "again1": a[:6], "again0": b[:6], "again_at": 33}


BUILDERS = {"short": (_short, True), "frozen": (_frozen, False), "bot": (_bot, True)}
Scenario = collections.namedtuple("Scenario", "name level n auto_reset events info seeds listed")
SEED_BASE = 515100


@functools.lru_cache(maxsize=None)
def scenario(name, level, n):
    build, auto = BUILDERS[name]
    events, info = build(level, n)
    listed = np.unique(np.concatenate([np.asarray(ev[1], np.int64) for ev in events if ev[0] == "reseed"]))
    return Scenario(name, level, n, auto, events, info, np.arange(n, dtype=np.uint64) + np.uint64(SEED_BASE), listed)


@functools.lru_cache(maxsize=None)
def model_run(name, level, n, done_actions=False):
    """The host model's outputs of a scenario: computed once per process, shared by every test, never written to."""
    sc = scenario(name, level, n)
    return ParkingModel(level, sc.seeds, auto_reset=sc.auto_reset, done_actions=done_actions).run(sc.events)


def twin_events(events):
    """The same script with every reseed at depth 0: what the twin handle plays."""
    return [ev[:3] + (0,) if ev[0] == "reseed" else ev for ev in events]


# ---- the device side ------------------------------------------------------------------------------------------------------------------
class WithLevels(object):
    """A BatchedBabyAIEnv whose reseed(ids, seeds) takes its `levels` from the script's reseed events, in order: scenario_util.run_device
    knows three-element reseed events only."""

    def __init__(self, env, events):
        self.__dict__["_env"] = env
        self.__dict__["_depths"] = collections.deque(int(ev[3]) if len(ev) > 3 else 0 for ev in events if ev[0] == "reseed")

    def __getattr__(self, name):
        return getattr(self._env, name)

    def __setattr__(self, name, value):
        setattr(self._env, name, value)

    def reseed(self, ids, seeds):
        return self._env.reseed(ids, seeds, levels=self._depths.popleft())


def assert_run(got, want, twin=False):
    """A device run (scenario_util.run_device) against the model's: every byte of every env that is not parked -- image, direction, token row
    --, and reward (f32 and f64 bits) and done of EVERY env: a parked env's stay what its last episode left.  bbai_bot_rollout's history
    rows: observation and token rows of the envs that are not parked in front of the step, action and gave_up of every env (a parked env:
    `done`, 0), reward and done of the envs that are not parked in front of the step (a frozen env's step writes neither, and a history row
    is a buffer of its own).  twin=True: `got` is the run of the twin handle, whose reseeds were all at depth 0 -- its envs never park and
    play on where the model's are parked, so EVERY output of an env is left out while the model has it parked."""
    assert got["T"] == want["T"], (got["T"], want["T"])
    after, before, calls = want["parked"], want["parked_before"], want["parked_calls"]
    what = "the model (twin handle, depth 0)" if twin else "the host model"
    masked = lambda k: twin or k in MASKED

    def same(label, g, w, keep=None):
        g, w = su._bits(np.asarray(g)), su._bits(np.asarray(w))
        assert g.shape == w.shape, (label, g.shape, w.shape)
        if keep is not None:
            g, w = g[keep], w[keep]
        if not np.array_equal(g, w):
            bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
            rows = np.flatnonzero(keep)[bad] if keep is not None else bad
            raise AssertionError("%s differs from %s in envs %s" % (label, what, rows[:12].tolist()))

    for k, rows in got["steps"].items():
        assert not rows or len(rows) == want["T"], (k, len(rows))
        for t, row in enumerate(rows):
            if row is not None:
                same("step %d %s" % (t, k), row, want["steps"][k][t], ~after[t] if masked(k) else None)
    for t, f in got["finals"].items():
        for k, v in f.items():
            same("buffer %s behind the rollout call that ends with step %d" % (k, t), v, want["steps"][k][t], ~after[t] if masked(k) else None)
    assert len(got["calls"]) == len(want["calls"]) == len(calls)
    for j, (c, w) in enumerate(zip(got["calls"], want["calls"])):
        for k in MASKED:
            if c[k] is not None:
                same("call %d %s" % (j, k), c[k], w[k], ~calls[j])
    if got["bot"]["action"] is not None:
        assert len(got["bot"]["action"]) == want["T"]          # (a bot script has no other steps: bot row t = step t)
        for k, v in got["bot"].items():
            for t in range(len(v)):
                same("bot_rollout step %d %s" % (t, k), v[t], want["bot"][k][t], None if k in ("action", "gave_up") and not twin else ~before[t])


def parked_facts(want, sc):
    """What the scenarios claim, from the model alone: (first parked step per env or -1, share of the listed envs' (env, step) pairs that are parked)."""
    p = want["parked"]
    first = np.where(p.any(axis=0), p.argmax(axis=0), -1)
    return first, float(p[:, sc.listed].mean())


# ---- the host build behind the pool schedulers' env protocols ---------------------------------------------------------------------------
class HostPoolLevels(HostPool):
    """seed_demos_util.HostPool on a ParkingModel: reseed honours `levels`, and bot_rollout leaves a parked env's reward / done history rows
    UNWRITTEN, as bbai_bot_rollout does -- here they keep the poison the slot was filled with, which says `done` on every row."""

    def __init__(self, level, seeds):
        super().__init__(level, seeds)
        self.model = ParkingModel(level, np.asarray(seeds, dtype=np.uint64), auto_reset=True)
        self.levels_seen, self.parked_rows = [], 0

    def bot_rollout(self, steps, tokens=False, out=None):
        m, hb = self.model, self.model.hb
        assert tokens and out is not None
        o = {k: v.numpy() for k, v in out.items()}
        o["done"][:], o["reward"][:] = 0xA5, np.float32(0.75)
        for t in range(steps):
            live = ~m.parked
            o["image"][t], o["direction"][t], o["tokens"][t] = hb.image, hb.direction, m.tokens()
            act, gave = m.bot_decide()
            m.step(act)
            o["action"][t], o["gave_up"][t] = act, gave
            o["reward"][t][live], o["done"][t][live] = hb.reward[live], hb.done[live]
            self.parked_rows += int((~live).sum())
        self.rollouts += 1
        return out

    def reseed(self, ids, seeds, levels=None):
        self.levels_seen.append(levels)
        self.model.reseed(ids.numpy(), seeds.numpy().view(np.uint64), levels=levels or 0)
        self.reseeds += 1


class HostEvalEnv(object):
    """What evaluate._evaluate_pool uses of a BatchedBabyAIEnv, on CPU tensors over a ParkingModel (auto_reset=False)."""
    made = []

    def __init__(self, env_name, n, device=None, pixel=False, auto_reset=False):
        import torch
        assert not auto_reset and not pixel
        self.level, self.num_envs, self.device = env_name[len("BabyAI-"):-len("-v0")], int(n), torch.device("cpu")
        self.levels_seen, self.closed = [], False
        HostEvalEnv.made.append(self)

    def seed(self, seeds):
        self.model = ParkingModel(self.level, np.asarray(seeds, dtype=np.uint64), auto_reset=False)

    def _sync(self):
        import torch
        hb = self.model.hb
        self.image.copy_(torch.as_tensor(hb.image)); self.direction.copy_(torch.as_tensor(hb.direction))
        self.instr.copy_(torch.as_tensor(self.model.tokens()))
        return {"image": self.image, "direction": self.direction}

    def enable_instr_tokens(self):
        import torch
        n = self.num_envs
        self.image, self.direction = torch.zeros((n, 7, 7, 3), dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8)
        self.instr = torch.zeros((n, su.TOK_MAX), dtype=torch.uint8)
        self.reward64, self.done = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.uint8)
        return self.instr

    def reset(self):
        return self._sync()          # (ScenarioModel is built behind its reset)

    def step(self, action):
        import torch
        self.model.step(action.numpy())
        self.reward64.copy_(torch.as_tensor(self.model.hb.reward64)); self.done.copy_(torch.as_tensor(self.model.hb.done))
        return self._sync(), self.reward64.to(torch.float32), self.done, {}

    def reseed(self, ids, seeds, levels=None):
        self.levels_seen.append(levels)
        self.model.reseed(ids.numpy(), np.asarray(seeds, dtype=np.uint64), levels=levels or 0)
        return self._sync()

    def close(self):
        self.closed = True
