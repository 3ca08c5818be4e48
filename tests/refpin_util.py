"""Protocols that run alike on the REFERENCE (tools/gen_golden_refpin.py records them once, where the reference tree can be
imported) and on this project's own code (the tests replay them and compare), and the digests that pin them.

The fixtures live in tests/golden/refpin/: a record per episode (mission, max_steps, steps taken, a sha256 digest over every
observation / direction / float64 reward / done the episode produced), the reference's level attributes, the vocabulary and
token ids of the reference's InstructionsPreprocessor, the experiences of the reference's BaseAlgo.collect_experiences, and the
answers of the reference's expert (babyai/bot.py) to the bot tests' questions, in call order (Recording / Replay).
The tests that once stepped the reference side by side with the oracle now step the oracle against these records -- same
seeds, same actions, the same equality, with no file outside the repository."""
import hashlib
import json
import os
import random

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refpin")


def golden_path(name):
    return os.path.join(GOLDEN, name)


def load_json(name):
    if name.endswith(".gz"):
        import gzip
        with gzip.open(golden_path(name), "rt") as f:
            return json.load(f)
    with open(golden_path(name)) as f:
        return json.load(f)


class Digest(object):
    """sha256 over arrays in a fixed dtype (uint8 images / grids, int64 directions, float64 rewards, uint8 dones)."""

    def __init__(self):
        self.h = hashlib.sha256()

    def add(self, a, dtype):
        a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
        self.h.update(repr(a.shape).encode())
        self.h.update(a.tobytes())

    def reset(self, obs, grid):
        self.add(obs["image"], np.uint8)
        self.add(grid.encode(), np.uint8)
        self.add(obs["direction"], np.int64)

    def step(self, obs, reward, done):
        self.add(obs["image"], np.uint8)
        self.add(obs["direction"], np.int64)
        self.add(reward, np.float64)
        self.add(bool(done), np.uint8)

    def hexdigest(self):
        return self.h.hexdigest()


def level_digest(grid, image, agent, max_steps, mission):
    """The level digest of tests/golden/refpin/gen_digest/: the first 4 bytes of sha256 (little endian, as a uint32) over
      - the grid after the reset, uint8[H][W], one byte per cell: type | color << 3 | state << 6;
      - the first observation, uint8[7][7][3] (on the *Carrying levels taken BEFORE the object moves into the agent's hands; the grid after);
      - agent x, y, dir, one byte each;
      - max_steps, 2 bytes little endian;
      - the mission string, UTF-8.
    Four producers feed it: a reference env (tools/gen_golden_refpin.py gen), an oracle env, the engine's host build and the engine."""
    grid, image = np.asarray(grid), np.asarray(image)
    assert grid.ndim == 2 and grid.dtype == np.uint8 and image.shape == (7, 7, 3) and image.dtype == np.uint8
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(grid).tobytes())
    h.update(np.ascontiguousarray(image).tobytes())
    h.update(bytes([int(agent[0]), int(agent[1]), int(agent[2])]))
    h.update(int(max_steps).to_bytes(2, "little"))
    h.update(mission.encode("utf-8"))
    return int.from_bytes(h.digest()[:4], "little")


def env_level_digest(env, obs):
    """level_digest of a reference or oracle env right after `obs = env.reset()`."""
    g = np.asarray(env.grid.encode())
    grid = (g[:, :, 0] | (g[:, :, 1] << 3) | (g[:, :, 2] << 6)).T.astype(np.uint8)
    return level_digest(grid, np.asarray(obs["image"], dtype=np.uint8), (env.agent_pos[0], env.agent_pos[1], env.agent_dir),
                        env.max_steps, obs["mission"])


def record_level_digests(cfg, rec, hot, image, missions=None):
    """uint32[N]: level_digest of every env of a batch in the engine's state format -- records uint8[N, rec_bytes], hot uint8[N, 16]
    (bytes 0, 1, 2 = agent x, y, dir; 6, 7 = max_steps), the first observations uint8[N, 7, 7, 3] -- as HostBatch holds it and as
    export_state() / env.image return it.  `missions`: the N strings (env.missions()); None = rendered from each record's program."""
    from babyai_amd.missions import prog_surface
    rec, hot, image = np.asarray(rec), np.asarray(hot).view(np.uint8).reshape(len(rec), -1), np.asarray(image)
    grids = rec[:, :cfg.ES * cfg.EH].reshape(-1, cfg.EH, cfg.ES)[:, 5:5 + cfg.H, 5:5 + cfg.W]
    out = np.zeros(len(rec), np.uint32)
    for i in range(len(rec)):
        m = missions[i] if missions is not None else prog_surface(rec[i, cfg.off_prog:cfg.off_prog + 112])
        out[i] = level_digest(grids[i], image[i], hot[i, :3], int(hot[i, 6]) | int(hot[i, 7]) << 8, m)
    return out


GEN_DIGEST_SEED0, GEN_DIGEST_SEEDS, GEN_DIGEST_LEVELS = 52000, 512, 6


def gen_digest_fixture(name):
    """uint32[512, 6]: the reference's level digests of kind `name`, seeds 52000 + i, six consecutive resets each."""
    return np.load(golden_path(os.path.join("gen_digest", name + ".npy")))


def digest_mismatch(name, got, want, what):
    """Raise with the number of (seed, level) pairs whose digests differ and the first few of them (got, want: uint32[n_seeds, n_levels])."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint32, (got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s %s: %d of %d digests differ from the reference's, first (seed, level) %s"
                             % (name, what, len(bad), got.size, [(GEN_DIGEST_SEED0 + int(i), int(k)) for i, k in bad[:8]]))


# ---- step digests: tests/golden/refpin/step_digest/<Level>.npz (tools/gen_golden_refpin.py step) --------------------------------
STEP_DIGEST_SEED0, STEP_DIGEST_STREAMS, STEP_DIGEST_BLOCK = 53000, 256, 16
STEP_DIGEST_OVERRIDE, STEP_DIGEST_BUDGET_S = 0.08, 2.0
STEP_ROW_BYTES = 147 + 1 + 8 + 1            # image uint8[7, 7, 3], direction, reward float64, done


# Kinds whose T was raised until 100 episodes ended in success: the reference's expert raises at the first decision of every episode that starts
# with the object in the agent's hands, so these streams run on random actions (at T = 320 they solved 63 and 46 episodes).
STEP_DIGEST_LONGER = {"PutNextS6N3Carrying": 640, "PutNextS7N4Carrying": 960}


def step_digest_steps(name):
    """T of a kind's streams: 128 steps in one room, 320 in several, more for STEP_DIGEST_LONGER (every T is a multiple of the 16-step block)."""
    from babyai_amd.levels import make_cfg
    cfg = make_cfg(name)
    return STEP_DIGEST_LONGER.get(name, 128 if cfg.num_rows * cfg.num_cols == 1 else 320)


def _digest32(rows):
    """uint32[n]: the first 4 bytes of sha256, little endian, of every row of the C-contiguous uint8[n, k]."""
    assert rows.dtype == np.uint8 and rows.ndim == 2 and rows.flags.c_contiguous
    return np.array([int.from_bytes(hashlib.sha256(r.data).digest()[:4], "little") for r in rows], np.uint32).reshape(len(rows))


def step_block_digests(image, direction, reward, done):
    """uint32[S, T // 16] from the outputs of T steps of S streams -- image uint8[T, S, 7, 7, 3], direction [T, S], reward [T, S] (taken as
    float64), done [T, S]: per stream and 16-step block the first 4 bytes of sha256 (little endian, as level_digest) over, step by step,
    the image (147 bytes), the direction (1 byte), the reward (float64, 8 bytes little endian) and done (1 byte)."""
    image, direction, reward, done = np.asarray(image), np.asarray(direction), np.asarray(reward), np.asarray(done)
    steps, n = direction.shape
    assert steps % STEP_DIGEST_BLOCK == 0 and image.shape == (steps, n, 7, 7, 3) and image.dtype == np.uint8, (image.shape, image.dtype)
    assert reward.shape == done.shape == (steps, n) and reward.dtype.kind == "f", (reward.shape, done.shape, reward.dtype)
    rows = np.zeros((n, steps, STEP_ROW_BYTES), np.uint8)
    rows[:, :, :147] = image.reshape(steps, n, 147).transpose(1, 0, 2)
    rows[:, :, 147] = direction.T
    rows[:, :, 148:156] = np.ascontiguousarray(reward.T.astype("<f8")).view(np.uint8).reshape(n, steps, 8)
    rows[:, :, 156] = done.T != 0
    return _digest32(rows.reshape(n * (steps // STEP_DIGEST_BLOCK), STEP_DIGEST_BLOCK * STEP_ROW_BYTES)).reshape(n, steps // STEP_DIGEST_BLOCK)


def step_first_digests(image, direction):
    """uint32[S]: the same digest of the first observation uint8[S, 7, 7, 3] and direction [S] of every stream."""
    image, direction = np.asarray(image), np.asarray(direction)
    assert image.shape == (len(direction), 7, 7, 3) and image.dtype == np.uint8
    rows = np.zeros((len(direction), 148), np.uint8)
    rows[:, :147] = image.reshape(-1, 147)
    rows[:, 147] = direction
    return _digest32(rows)


def pack_actions(actions):
    """uint8[T, S] with values <= 15 -> uint8[T, S // 2]: stream 2k in the low half of byte k, stream 2k + 1 in the high half."""
    a = np.asarray(actions, np.uint8)
    assert a.ndim == 2 and a.shape[1] % 2 == 0 and a.max() <= 15
    return a[:, 0::2] | (a[:, 1::2] << 4)


def unpack_actions(packed):
    p = np.asarray(packed, np.uint8)
    a = np.zeros((p.shape[0], p.shape[1] * 2), np.uint8)
    a[:, 0::2], a[:, 1::2] = p & 15, p >> 4
    return a


def pack_bits(bits):
    """bool[T, S] -> uint8[T, S // 8] (numpy's packbits, the first stream in the top bit)."""
    return np.packbits(np.asarray(bits).astype(bool), axis=1)


def unpack_bits(packed, n):
    return np.unpackbits(np.asarray(packed, np.uint8), axis=1)[:, :n].astype(bool)


class RecordedActions(object):
    """The policy of a replay: the stored actions of one stream, whatever the env shows."""

    def __init__(self, actions):
        self.actions = actions

    def episode(self, env):
        pass

    def act(self, t):
        return int(self.actions[t]), False, False


def step_digest_stream(env, steps, policy):
    """One stream of the step-digest protocol on a seeded level object (the reference's, the oracle's): reset(), then `steps` steps with the
    engine's auto-reset semantics -- on done the env is reset at once and the step's output observation is the new episode's first one (on the
    *Carrying kinds reset() returns it from before the object moves into the agent's hands).  policy.episode(env) is called after every
    reset, policy.act(t) -> (action, was the expert's own suggestion, expert dead) before every step.
    Returns a dict: first_image, first_direction, image uint8[steps, 7, 7, 3], direction, reward (float64), done, action, suggested,
    bot_dead, and ends = [successes, failures before the time limit, time limits]."""
    out = {"image": np.zeros((steps, 7, 7, 3), np.uint8), "direction": np.zeros(steps, np.uint8), "reward": np.zeros(steps, np.float64),
           "done": np.zeros(steps, np.uint8), "action": np.zeros(steps, np.uint8), "suggested": np.zeros(steps, bool),
           "bot_dead": np.zeros(steps, bool), "ends": np.zeros(3, np.int64)}
    obs = env.reset()
    out["first_image"], out["first_direction"] = np.asarray(obs["image"], np.uint8), int(obs["direction"])
    policy.episode(env)
    for t in range(steps):
        a, out["suggested"][t], out["bot_dead"][t] = policy.act(t)
        out["action"][t] = a
        obs, reward, done, _ = env.step(a)
        if done:
            out["ends"][0 if reward > 0 else 1 if env.step_count < env.max_steps else 2] += 1
            obs = env.reset()
            policy.episode(env)
        out["image"][t], out["direction"][t], out["reward"][t], out["done"][t] = obs["image"], obs["direction"], reward, done
    return out


def step_digest_run(env_for_seed, streams, steps, policy_for_stream):
    """step_digest_stream on the streams `streams` (stream i: env_for_seed(53000 + i), policy_for_stream(i)) -> their outputs stacked
    with the stream as the second axis ([steps, k, ...]; first_image [k, 7, 7, 3], ends [k, 3]), as step_block_digests takes them."""
    runs = [step_digest_stream(env_for_seed(STEP_DIGEST_SEED0 + i), steps, policy_for_stream(i)) for i in streams]
    out = {k: np.stack([r[k] for r in runs], axis=1) for k in ("image", "direction", "reward", "done", "action", "suggested", "bot_dead")}
    for k in ("first_image", "first_direction", "ends"):
        out[k] = np.stack([np.asarray(r[k]) for r in runs])
    return out


def step_digest_fixture(name):
    """The recorded file of kind `name`, unpacked: actions uint8[T, S], digest uint32[S, T // 16], first uint32[S], suggested / bot_dead
    bool[T, S], budget int32[k, 2] = the (step, stream) pairs at which the expert's death was the decision budget and not an exception
    of the reference's, ends int64[S, 3]."""
    with np.load(golden_path(os.path.join("step_digest", name + ".npz"))) as z:
        n = int(z["digest"].shape[0])
        return {"actions": unpack_actions(z["actions"]), "digest": z["digest"], "first": z["first"],
                "suggested": unpack_bits(z["suggested"], n), "bot_dead": unpack_bits(z["bot_dead"], n), "budget": z["budget"], "ends": z["ends"]}


def step_digest_mismatch(name, got_first, got, fx, what, streams=None):
    """Raise with the number of (stream, block) pairs whose digests differ from the recording and the first few (block -1 = the first
    observation).  `streams`: the streams got_first [k] / got [k, T // 16] hold (default: all, in order)."""
    streams = np.arange(len(fx["first"])) if streams is None else np.asarray(streams)
    want_first, want = fx["first"][streams], fx["digest"][streams]
    got_first, got = np.asarray(got_first), np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint32 == got_first.dtype, (got.shape, want.shape, got.dtype, got_first.dtype)
    if not (np.array_equal(got_first, want_first) and np.array_equal(got, want)):
        bad = [(int(streams[i]), -1) for i in np.nonzero(got_first != want_first)[0]] + [(int(streams[i]), int(b)) for i, b in np.argwhere(got != want)]
        raise AssertionError("%s %s: %d of %d (stream, block) digests differ from the reference's, first %s (steps %d .. %d of stream %d)"
                             % (name, what, len(bad), got.size + got_first.size, sorted(bad)[:8], max(sorted(bad)[0][1], 0) * STEP_DIGEST_BLOCK,
                                max(sorted(bad)[0][1], 0) * STEP_DIGEST_BLOCK + STEP_DIGEST_BLOCK - 1, sorted(bad)[0][0]))


def step_digest_expert(name, what, suggestion, done, fx, streams=None):
    """An expert's answers on a replay of the recording -- suggestion uint8[T, k] before every step (255: it gave up), done [T, k] of the
    replay (equal to the reference's once the digests are) -- against the reference expert's: the recorded action wherever the recording
    says it was the expert's own suggestion, and 255 at the step of every episode at which the reference's expert first was dead because it
    RAISED.  Deaths by the decision budget (fx["budget"]) are no statement about the expert and are left out.
    Returns (decisions compared, deaths compared)."""
    streams = np.arange(len(fx["first"])) if streams is None else np.asarray(streams)
    suggestion, done = np.asarray(suggestion), np.asarray(done) != 0
    dead, acts = fx["bot_dead"][:, streams], fx["actions"][:, streams]
    own = fx["suggested"][:, streams] & ~dead
    bad = np.argwhere(own & (suggestion != acts))
    assert len(bad) == 0, "%s %s: the expert differs from the reference's at %d (step, stream) pairs, first (step, stream, got, want) %s" % (
        name, what, len(bad), [(int(t), int(streams[i]), int(suggestion[t, i]), int(acts[t, i])) for t, i in bad[:8]])
    raised = dead.copy()
    raised[1:] &= ~dead[:-1] | done[:-1]                 # the first dead step of an episode
    pos = {int(s): k for k, s in enumerate(streams)}
    for t, i in fx["budget"]:
        if int(i) in pos:
            raised[t, pos[int(i)]] = False
    bad = np.argwhere(raised & (suggestion != 255))
    assert len(bad) == 0, "%s %s: the reference's expert raised where this one suggests, at %d (step, stream) pairs, first (step, stream, got) %s" % (
        name, what, len(bad), [(int(t), int(streams[i]), int(suggestion[t, i])) for t, i in bad[:8]])
    return int(own.sum()), int(raised.sum())


def reference_level(level_dict, name, **kw):
    """A reference level object as the tests always built it: without the stale `locked_room` the reference's entropy-seeded
    constructor leaves behind (tools/gen_golden.py)."""
    env = level_dict[name](**kw)
    if hasattr(env, "locked_room"):
        env.locked_room = None
    return env


def random_episodes(env_for_seed):
    """tests/test_oracle_reference.py's protocol: seeds 2 and 9, two episodes each, up to 250 uniformly random actions
    (random.Random(seed).randint(0, 6)).  `env_for_seed(seed)` returns a seeded level object."""
    recs = []
    for seed in (2, 9):
        env = env_for_seed(seed)
        rng = random.Random(seed)
        for ep in range(2):
            obs = env.reset()
            d = Digest()
            d.reset(obs, env.grid)
            rec = {"seed": seed, "ep": ep, "mission": obs["mission"], "max_steps": int(env.max_steps)}
            for t in range(250):
                obs, reward, done, _ = env.step(rng.randint(0, 6))
                d.step(obs, reward, done)
                if done:
                    break
            rec["steps"] = t + 1
            rec["digest"] = d.hexdigest()
            recs.append(rec)
    return recs


STRICT_CASES = [
    ("PutNextLocal", True, False),           # PutNext strict: any pickup that leaves the agent holding something fails
    ("PutNextS5N2", True, False),
    ("GoToSeqS5R2", False, True),            # Before / After strict: completing the second part first fails
    ("SynthSeq", False, True),               # ... with And sides: the probe's side effects (progress bits, preCarrying)
    ("MiniBossLevel", True, True),           # everything at once
]


def strict_episodes(env_for_seed, arm, twin=None):
    """tests/test_strict_modes.py's protocol: seeds 0..11, three episodes each, strict switched on by `arm(env)` after every
    reset, up to 400 actions from random.Random(seed * 7 + 1).  `twin(seed)`, when given, is a second implementation stepped
    alongside: twin.reset(obs) after every reset (before arm), twin.step(act, obs, reward, done) after every step -- it
    asserts its own equality.  One record per episode; `strict_failure` = the episode failed before its time limit."""
    recs = []
    for seed in range(12):
        env = env_for_seed(seed)
        tw = twin(seed) if twin is not None else None
        rng = random.Random(seed * 7 + 1)
        for ep in range(3):
            obs = env.reset()
            if tw is not None:
                tw.reset(obs)
            arm(env)
            d = Digest()
            d.reset(obs, env.grid)
            rec = {"seed": seed, "ep": ep, "mission": obs["mission"], "strict_failure": False}
            for t in range(400):
                act = rng.choice([0, 1, 2, 2, 2, 3, 3, 4, 5, 6])
                obs, reward, done, _ = env.step(act)
                if tw is not None:
                    tw.step(act, obs, reward, done)
                d.step(obs, reward, done)
                if done:
                    rec["strict_failure"] = bool(reward == 0 and env.step_count < env.max_steps)
                    break
            rec["steps"] = t + 1
            rec["digest"] = d.hexdigest()
            recs.append(rec)
    return recs


# the constructor attributes tests/test_oracle_reference.py reads off a reference level object (those it has)
LEVEL_ATTRS = ("room_size", "num_rows", "num_cols", "objs_per_room", "num_doors", "debug", "start_carrying", "action_kinds",
               "instr_kinds", "locked_room_prob", "num_dists", "locations", "unblocking", "implicit_unlock", "num_objs")


def level_attrs(env):
    out = {}
    for k in LEVEL_ATTRS:
        if hasattr(env, k):
            v = getattr(env, k)
            out[k] = list(v) if isinstance(v, (list, tuple)) else (v.item() if isinstance(v, np.generic) else v)
    return out


def vocab_missions():
    """tests/test_vocab_remap.py's 10^4 missions: three resets of every level in turn (the engine's host build), seeds 31000 + k."""
    from babyai_amd.levels import LEVELS, make_cfg
    from hostsim_util import HostEnv
    missions = []
    names = sorted(LEVELS)
    k = 0
    while len(missions) < 10000:
        h = HostEnv(make_cfg(names[k % len(names)]), 31000 + k)
        for _ in range(3):
            h.reset()
            missions.append(h.mission)
        k += 1
    return missions


def missions_digest(missions):
    return hashlib.sha256("\n".join(missions).encode()).hexdigest()


ROLLOUT_CASES = [("GoToObjS4", 16.0), ("GoToLocalS5N2", 16.0), ("GoToObjS4", 20.0)]
ROLLOUT_FIELDS = ("memory", "mask", "action", "value", "reward", "advantage", "returnn", "log_prob")
ROLLOUT_SEEDS = [500 + i for i in range(5)]
ROLLOUT_T = 24
ROLLOUT_ITERS = 3


def rollout_key(level, scale, it, field):
    return "%s_%g_%d_%s" % (level, scale, it, field)


def budgeted_replan(bot, last, budget_s):
    """(bot.replan(last), None), or (None, "raised") when the reference's expert raised, (None, "budget") when it took longer than budget_s."""
    import signal

    class Timeout(BaseException):
        pass

    def on_alarm(signum, frame):
        raise Timeout()
    try:
        signal.signal(signal.SIGALRM, on_alarm)
        signal.setitimer(signal.ITIMER_REAL, budget_s)
        try:
            return int(bot.replan(last)), None
        finally:
            signal.setitimer(signal.ITIMER_REAL, 0)
    except BaseException as exc:
        if isinstance(exc, KeyboardInterrupt):
            raise
        return None, "budget" if isinstance(exc, Timeout) else "raised"


class ExpertPolicy(object):
    """The recording policy of the step digests: a fresh reference Bot per episode, told the action taken; its suggestion overridden with
    probability 0.08 by rng.randint(0, 6) (rng = random.Random(seed), one per stream); every replan under the 2 s budget.  A bot that raised
    or ran out of budget is dead for the rest of the episode and the stream draws every action from rng.  `budget`: the steps at which
    the death was the budget's."""

    def __init__(self, Bot, seed):
        self.Bot, self.rng, self.budget = Bot, random.Random(seed), []

    def episode(self, env):
        self.bot, self.last = self.Bot(env), None

    def act(self, t):
        if self.bot is not None:
            sug, why = budgeted_replan(self.bot, self.last, STEP_DIGEST_BUDGET_S)
            if sug is None:
                self.bot = None
                if why == "budget":
                    self.budget.append(t)
        if self.bot is None:
            self.last = self.rng.randint(0, 6)
            return self.last, False, True
        self.last = self.rng.randint(0, 6) if self.rng.random() < STEP_DIGEST_OVERRIDE else sug
        return self.last, self.last == sug, False


class LiveBotRef(object):
    """The reference's level and its expert (babyai/bot.py), answering the questions tests/test_hostsim_bot.py asks of them."""

    def __init__(self):
        from babyai.bot import Bot
        from babyai.levels import level_dict
        self.Bot, self.level_dict = Bot, level_dict

    def make(self, level, seed, how):
        """how: "seed" = Level(), no stale locked_room, .seed(seed), reset(); "seed_keep" = the same with the constructor's
        locked_room left as it is; "ctor" = Level(seed=seed) (generated by the constructor, no reset)."""
        if how == "ctor":
            self.env = self.level_dict[level](seed=seed)
            return None
        self.env = reference_level(self.level_dict, level) if how == "seed" else self.level_dict[level]()
        self.env.seed(seed)
        self.env.reset()
        return None

    def new_bot(self):
        self.bot = self.Bot(self.env)
        return None

    def replan(self, last=None, budget_s=None):
        """The bot's next action; None when it raised or (budget_s) took longer than that."""
        if budget_s is None:
            return int(self.bot.replan(last))
        return budgeted_replan(self.bot, last, budget_s)[0]

    def step(self, action):
        _, reward, done, _ = self.env.step(action)
        return [float(reward), bool(done)]

    def reset(self):
        self.env.reset()
        return None

    def stack_depth(self):
        return len(self.bot.stack)


class Recording(object):
    """Forwards every call to `side` and logs [method, answer] (tools/gen_golden_refpin.py)."""

    def __init__(self, side):
        self.side, self.log = side, []

    def __getattr__(self, name):
        fn = getattr(self.side, name)

        def call(*args, **kw):
            v = fn(*args, **kw)
            self.log.append([name, v])
            return v
        return call


class Replay(object):
    """Answers the calls a Recording logged, in the same order (the tests); a call out of order is a failure."""

    def __init__(self, log):
        self.log, self.i = log, 0

    def __getattr__(self, name):
        def call(*args, **kw):
            assert self.i < len(self.log), "more calls than the recording holds"
            method, v = self.log[self.i]
            assert method == name, (self.i, method, name)
            self.i += 1
            return v
        return call

    def finished(self):
        return self.i == len(self.log)
