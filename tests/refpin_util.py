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
        import signal

        class Timeout(BaseException):
            pass

        def on_alarm(signum, frame):
            raise Timeout()
        try:
            signal.signal(signal.SIGALRM, on_alarm)
            signal.setitimer(signal.ITIMER_REAL, budget_s)
            try:
                return int(self.bot.replan(last))
            finally:
                signal.setitimer(signal.ITIMER_REAL, 0)
        except BaseException as exc:
            if isinstance(exc, KeyboardInterrupt):
                raise
            return None

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
