"""Helpers of tests/test_demo_replay_host.py and tests/test_gpu_demo_replay.py.  Every expected value of a replay comes from ONE plain model
(`model`): a single hostsim_util.HostEnv(make_cfg(level), seed), reset, then stepped with the demo's actions one by one, comparing as it goes --
no pool, no hold, no reseed.  Next to it: the host build behind the tensor protocol that `DemoStore.replay(env=...)` drives (HostReplayPool),
stores built from seed_demos_util's expert episodes or from random-action episodes, the ways to make such a store wrong, and synthetic
pools with plain loops for `replay_feed` / `replay_judge`.  Everything is computed once per process and never written to."""
import functools

import numpy as np
import torch

import seed_demos_util as sd
from babyai_amd import missions
from babyai_amd.imitation import DemoStore
from babyai_amd.levels import make_cfg
from hostsim_util import HostEnv
from scenario_util import ScenarioModel

TOK_MAX = 72
HOLD = 8
FIELDS = ("played", "done_at", "return64", "mismatches", "first_mismatch", "mission_ok")
# (level, first seed, one past the last, demos, frames): the issue's cases of the whole loop; the figures are recomputed and asserted
LOOP_CASES = {"GoToLocal": ("GoToLocal", 1000, 1024, 24, 125), "PutNextLocal": ("PutNextLocal", 1000, 1024, 24, 336),
              "BossLevel": ("BossLevel", 1000, 1012, 12, 1189)}


# ---- the plain model --------------------------------------------------------------------------------------------------------------------
def model(level, seed, tokens, images, dirs, actions):
    """One demo (token row uint8[72], images uint8[L, 7, 7, 3], directions, actions) played back in the episode of `seed` -> its results."""
    env = HostEnv(make_cfg(level), int(seed))
    img = env.reset()
    ids = missions.tokenize(env.mission)[:TOK_MAX]
    tok = np.zeros(TOK_MAX, np.uint8)
    tok[:len(ids)] = ids
    out = {"played": 0, "done_at": 0, "return64": 0.0, "mismatches": 0, "first_mismatch": -1,
           "mission_ok": int(len(actions) > 0 and np.array_equal(tok, tokens))}
    for t in range(len(actions)):
        if not np.array_equal(img, images[t]) or env.agent[2] != int(dirs[t]):
            out["mismatches"] += 1
            if out["first_mismatch"] < 0:
                out["first_mismatch"] = t
        img, _, done = env.step(int(actions[t]))
        out["played"] = t + 1
        if done:
            out["done_at"], out["return64"] = t + 1, env.last_reward64
            break
    return out


def model_store(level, seeds, arrays):
    """The model over a whole store given as arrays (dict of image / direction / action / tokens / offset) -> dict of result arrays."""
    off = arrays["offset"]
    rows = [model(level, s, arrays["tokens"][k], arrays["image"][off[k]:off[k + 1]], arrays["direction"][off[k]:off[k + 1]],
                  arrays["action"][off[k]:off[k + 1]]) for k, s in enumerate(seeds)]
    dt = {"return64": np.float64, "mission_ok": np.uint8}
    return {f: np.array([r[f] for r in rows], dtype=dt.get(f, np.int32)) for f in FIELDS}


def assert_replay_is(rep, want, arrays):
    lens = np.diff(arrays["offset"])
    for f in FIELDS:
        got = getattr(rep, f).cpu().numpy()
        assert got.dtype == want[f].dtype and got.shape == want[f].shape, f
        if f == "return64":
            assert np.array_equal(got.view(np.uint64), want[f].view(np.uint64)), (f, got, want[f])          # bit for bit
        else:
            assert np.array_equal(got, want[f]), (f, got, want[f])
    exact = (want["done_at"] == lens) & (want["mismatches"] == 0) & (want["mission_ok"] != 0)
    assert np.array_equal(rep.exact.cpu().numpy(), exact)
    assert np.array_equal(rep.length.cpu().numpy(), lens)
    return exact


# ---- stores -----------------------------------------------------------------------------------------------------------------------------
def as_store(arrays, device="cpu"):
    image, direction, action, tokens = (np.array(arrays[k]) for k in ("image", "direction", "action", "tokens"))       # (copies: the cases are read-only)
    return DemoStore._from_arrays(image, direction, action, tokens, np.array(arrays["offset"]), device)


@functools.lru_cache(maxsize=None)
def expert_case(name):
    """(level, seeds of the kept demos, the store's arrays) of a LOOP_CASES entry: the expert's demonstrations (seed_demos_util.expected)."""
    level, lo, hi, demos, frames = LOOP_CASES[name]
    seeds = tuple(range(lo, hi))
    want = sd.expected(level, seeds)
    assert len(want["kept"]) == len(seeds) == demos and int(want["offset"][-1]) == frames          # every listed seed is kept
    return level, np.array(seeds, dtype=np.uint64), {k: want[k] for k in ("image", "direction", "action", "tokens", "offset")}


@functools.lru_cache(maxsize=None)
def random_case(level="PutNextS5N2Carrying", lo=2000, count=24):
    """Random-action episodes recorded from HostEnv until `done`: a store that is not the expert's (level, seeds, arrays, returns)."""
    rng = np.random.default_rng(11)
    image, direction, action, tokens, lens, returns = [], [], [], [], [], []
    for s in range(lo, lo + count):
        env = HostEnv(make_cfg(level), s)
        img = env.reset()
        ids = missions.tokenize(env.mission)[:TOK_MAX]
        tok = np.zeros(TOK_MAX, np.uint8)
        tok[:len(ids)] = ids
        tokens.append(tok)
        n = 0
        while True:
            a = int(rng.integers(0, 6))
            image.append(img)
            direction.append(env.agent[2])
            action.append(a)
            img, _, done = env.step(a)
            n += 1
            if done:
                break
        lens.append(n)
        returns.append(env.last_reward64)
    arrays = {"image": np.stack(image), "direction": np.array(direction, np.uint8), "action": np.array(action, np.uint8),
              "tokens": np.stack(tokens), "offset": np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)}
    for a in arrays.values():
        a.setflags(write=False)
    return level, np.arange(lo, lo + count, dtype=np.uint64), arrays, np.array(returns)


def edited(arrays, **changes):
    """A writable copy of a store's arrays with some of them replaced."""
    out = {k: v.copy() for k, v in arrays.items()}
    out.update(changes)
    return out


def resized(arrays, demo, delta):
    """Demo `demo` cut short by its last -delta frames (delta < 0) or with `delta` frames appended behind its end (copies of its last frame,
    action 0)."""
    off = arrays["offset"]
    lo, hi = int(off[demo]), int(off[demo + 1])
    out = {"tokens": arrays["tokens"].copy(), "offset": off.copy()}
    out["offset"][demo + 1:] += delta
    for k in ("image", "direction", "action"):
        a = arrays[k]
        if delta < 0:
            out[k] = np.concatenate([a[:hi + delta], a[hi:]])
        else:
            pad = np.repeat(a[hi - 1:hi], delta, axis=0)
            if k == "action":
                pad[:] = 0
            out[k] = np.concatenate([a[:hi], pad, a[hi:]])
    return out


def with_empty_demo(arrays, at):
    """A zero-length demo put in front of demo `at`."""
    out = {k: arrays[k].copy() for k in ("image", "direction", "action")}
    out["tokens"] = np.insert(arrays["tokens"], at, np.zeros(TOK_MAX, np.uint8), axis=0)
    out["offset"] = np.insert(arrays["offset"], at, arrays["offset"][at])
    return out


# ---- the host build behind replay's env protocol --------------------------------------------------------------------------------------
class HostReplayPool(object):
    """ScenarioModel with auto_reset=False as the `env=` of DemoStore.replay: CPU tensors that share the model's arrays.  HOLD is modelled by
    saving and restoring the held envs' rows around the host build's step."""
    HELD_ROWS = ("mt", "mti", "rec", "hot", "stale", "image", "direction", "reward64", "done")

    def __init__(self, level, seeds, done_actions=False):
        self.model = ScenarioModel(level, np.asarray(seeds, dtype=np.uint64), auto_reset=False)
        self.done_actions = bool(done_actions)
        self.num_envs, self.device = self.model.n, torch.device("cpu")
        self.steps = self.reseeds = self.stepped_envs = 0
        self.closed = False

    image = property(lambda self: torch.from_numpy(self.model.hb.image))
    direction = property(lambda self: torch.from_numpy(self.model.hb.direction))
    reward64 = property(lambda self: torch.from_numpy(self.model.hb.reward64))
    done = property(lambda self: torch.from_numpy(self.model.hb.done))
    instr = property(lambda self: torch.from_numpy(self.model.tokens()))

    def step(self, actions):
        hb = self.model.hb
        act = actions.numpy().copy()
        assert act.shape == (self.num_envs,) and (act <= HOLD).all()
        held = np.flatnonzero(act == HOLD)
        live = act != HOLD
        assert not (hb.hot[live, 13] != 0).any()         # replay never steps a finished env
        saved = {k: getattr(hb, k)[held].copy() for k in self.HELD_ROWS}
        act[held] = 0
        self.model.step(act)
        for k, v in saved.items():
            getattr(hb, k)[held] = v
        self.steps += 1
        self.stepped_envs += int(live.sum())

    def reseed(self, ids, seeds, levels=None):
        assert levels == 1
        self.model.reseed(ids.numpy(), seeds.numpy().view(np.uint64))
        self.reseeds += 1

    def close(self):
        self.closed = True


def host_replay(level, seeds, arrays, pool, **kw):
    """DemoStore.replay on the host build: a pool of min(pool, non-empty demos) envs on the first of their seeds."""
    store = as_store(arrays)
    jobs = np.flatnonzero(np.diff(arrays["offset"]) > 0)
    env = HostReplayPool(level, np.asarray(seeds, dtype=np.uint64)[jobs][:min(pool, len(jobs))])
    rep = store.replay("BabyAI-%s-v0" % level, seeds, env=env, **kw)
    assert not env.closed
    return rep, env


# ---- synthetic pools for replay_feed ----------------------------------------------------------------------------------------------------
FEED_POOLS = (1, 63, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def feed_case(n):
    """A store of random frames and `calls` feeds of a pool of n envs whose observations are copies of the frames they stand at, with planted
    differences: image byte 0 only, byte 146 only, the direction only, the token row at pos == 0, the token row at pos > 0 (ignored); envs
    that are idle, stand at pos == length, at a negative pos or hold a job outside the store.  -> the calls' inputs and, from a plain loop,
    the outputs and the running results after every call."""
    rng = np.random.default_rng(500 + n)
    D = n + 5
    lens = rng.integers(1, 7, size=D)
    lens[rng.integers(0, D)] = 0
    if n == 1:
        lens = np.array([3, 0, 6, 5, 4, 2])     # 20 frames: the 24 calls below walk through all of them in steps of 7
    off =np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    F = int(off[-1])
    arrays = {"image": rng.integers(0, 256, (F, 7, 7, 3), dtype=np.uint8), "direction": rng.integers(0, 4, F, dtype=np.uint8),
              "action": rng.integers(0, 7, F, dtype=np.uint8), "tokens": rng.integers(0, 256, (D, TOK_MAX), dtype=np.uint8), "offset": off}
    res = {"mismatches": np.zeros(D, np.int32), "first_mismatch": np.full(D, -1, np.int32), "mission_ok": np.zeros(D, np.uint8)}
    calls, frames_fed, kinds = [], set(), set()
    for c in range(24 if n == 1 else 6):
        job = rng.permutation(D)[:n].astype(np.int32)
        pos = np.array([rng.integers(0, max(1, lens[j])) for j in job], dtype=np.int32)
        if n == 1:
            job[0], pos[0] = [(j, p) for j in range(D) for p in range(lens[j])][c * 7 % F]          # walk through the frames
        roles = rng.permutation(n)
        role = {}
        if n >= 63:
            names = ["idle", "used_up", "negative_pos", "job_beyond", "job_huge", "byte0", "byte146", "dir", "tok0", "tok_later", "two_bytes", "at0"]
            role = {nm: int(roles[k]) for k, nm in enumerate(names)}
            job[role["idle"]] = -1
            pos[role["used_up"]] = lens[job[role["used_up"]]]
            pos[role["negative_pos"]] = -1
            job[role["job_beyond"]] = D
            job[role["job_huge"]] = 0x7fffffff
            pos[role["tok0"]] = pos[role["at0"]] = 0
            if lens[job[role["tok_later"]]] < 2:
                job[role["tok_later"]] = -1
            else:
                pos[role["tok_later"]] = lens[job[role["tok_later"]]] - 1
        image, direction = np.zeros((n, 7, 7, 3), np.uint8), np.zeros(n, np.uint8)
        instr = rng.integers(0, 256, (n, TOK_MAX), dtype=np.uint8)
        playing = np.zeros(n, bool)
        for i in range(n):
            j, p = int(job[i]), int(pos[i])
            if 0 <= j < D and 0 <= p < lens[j]:
                playing[i] = True
                image[i], direction[i], instr[i] = arrays["image"][off[j] + p], arrays["direction"][off[j] + p], arrays["tokens"][j]
            else:
                image[i] = rng.integers(0, 256, (7, 7, 3), dtype=np.uint8)
        flat = image.reshape(n, 147)
        for nm, i in role.items():
            if not playing[i]:
                continue
            kinds.add(nm)
            if nm in ("byte0", "two_bytes"):
                flat[i, 0] ^= 0x10
            if nm in ("byte146", "two_bytes"):
                flat[i, 146] ^= 0x01
            if nm == "dir":
                direction[i] ^= 1
            if nm in ("tok0", "tok_later"):
                instr[i, 71 if c % 2 else 0] ^= 0x80
        if n == 1 and c % 3 == 1:
            flat[0, (c * 31) % 147] ^= 0xff
        actions, fed = np.full(n, HOLD, np.uint8), np.zeros(n, np.uint8)
        for i in range(n):                      # the plain loop
            if not playing[i]:
                continue
            j, p = int(job[i]), int(pos[i])
            f = int(off[j]) + p
            frames_fed.add(f)
            if not np.array_equal(image[i], arrays["image"][f]) or direction[i] != arrays["direction"][f]:
                res["mismatches"][j] += 1
                if res["first_mismatch"][j] < 0:
                    res["first_mismatch"][j] = p
            if p == 0:
                res["mission_ok"][j] = int(np.array_equal(instr[i], arrays["tokens"][j]))
            actions[i], fed[i] = arrays["action"][f], 1
        calls.append({"job": job, "pos": pos, "image": image, "direction": direction, "instr": instr, "actions": actions, "fed": fed,
                      "results": {k: v.copy() for k, v in res.items()}, "roles": role})
    return {"arrays": arrays, "calls": calls, "phases": {(147 * f) % 16 for f in frames_fed}, "kinds": kinds, "D": D}


def feed_run(case, device):
    """The calls of a feed case through imitation.replay_feed on `device` -> per call (actions, fed, results) as numpy."""
    from babyai_amd.imitation import replay_feed
    store = as_store(case["arrays"], device)
    D = case["D"]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)
    mism, first, ok = torch.zeros(D, dtype=torch.int32, device=device), torch.full((D,), -1, dtype=torch.int32, device=device), torch.zeros(D, dtype=torch.uint8, device=device)
    out = []
    for c in case["calls"]:
        n = len(c["job"])
        actions, fed = torch.full((n,), 77, dtype=torch.uint8, device=device), torch.full((n,), 77, dtype=torch.uint8, device=device)
        replay_feed(t(c["image"]), t(c["direction"]), t(c["instr"]), t(c["job"]), t(c["pos"]), store, mism, first, ok, actions, fed)
        out.append({"actions": actions.cpu().numpy().copy(), "fed": fed.cpu().numpy().copy(),
                    "results": {"mismatches": mism.cpu().numpy().copy(), "first_mismatch": first.cpu().numpy().copy(), "mission_ok": ok.cpu().numpy().copy()}})
    return out


def assert_feed(case, got):
    for c, (g, w) in enumerate(zip(got, case["calls"])):
        assert np.array_equal(g["actions"], w["actions"]) and np.array_equal(g["fed"], w["fed"]), c
        for k, v in w["results"].items():
            assert np.array_equal(g["results"][k], v), (c, k)


# ---- synthetic pools for replay_judge ---------------------------------------------------------------------------------------------------
JUDGE_POOLS = (1, 63, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def judge_case(n, calls=6):
    """`calls` judge calls in a row for a pool of n envs: done on fed and on unfed envs, demos used up without done, claim 0 / 1, a job list
    that runs out in the middle of a call and a cursor that ends above it.  The plain loop hands positions out in env order."""
    rng = np.random.default_rng(900 + n)
    live = max(1, n - n // 8)
    J = live + n // 2 + (2 if n == 1 else 0)   # the list runs out inside the second claiming call (nearly every env is free by then)
    D = J + 3
    lens = rng.integers(1, 5, size=D)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    job_demo = rng.permutation(D)[:J].astype(np.int32)
    job_seeds = rng.integers(0, 1 << 63, size=J, dtype=np.uint64)
    job, pos = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    job[:live] = job_demo[:live]
    res = {"played": np.full(D, -5, np.int32), "done_at": np.full(D, -5, np.int32), "return64": np.full(D, -5.0)}
    counters = np.array([live, 0], np.int64)
    out = []
    for c in range(calls):
        claim = c % 2 == 1
        before = {"job": job.copy(), "pos": pos.copy(), "counters": counters.copy(), "results": {k: v.copy() for k, v in res.items()}}
        fed = ((job >= 0) & (rng.random(n) < 0.8)).astype(np.uint8)
        if c == 0 and n > 8:
            fed[n - 1] = 1                      # "fed" without a job: skipped
        done = (rng.random(n) < (0.9 if c == 2 else 0.4)).astype(np.uint8)
        reward64 = rng.random(n) * (rng.random(n) < 0.7)
        fin = np.zeros(n, bool)
        ids, seeds = np.full(n, -1, np.int64), np.zeros(n, np.uint64)
        for i in range(n):
            j = int(job[i])
            if fed[i] and j >= 0:
                pos[i] += 1
                if done[i] or pos[i] >= lens[j]:
                    res["played"][j] = pos[i]
                    res["done_at"][j] = pos[i] if done[i] else 0
                    res["return64"][j] = reward64[i] if done[i] else 0.0
                    job[i] = -1
                    fin[i] = True
                    counters[1] += 1
            if claim and job[i] < 0:
                k = int(counters[0])
                counters[0] += 1
                if k < J:
                    job[i], pos[i], ids[i], seeds[i] = job_demo[k], 0, i, job_seeds[k]
        out.append({"claim": claim, "fed": fed, "done": done, "reward64": reward64, "before": before, "fin": fin, "ids": ids, "seeds": seeds,
                    "job": job.copy(), "pos": pos.copy(), "counters": counters.copy(), "results": {k: v.copy() for k, v in res.items()}})
    return {"calls": out, "offset": off, "job_demo": job_demo, "job_seeds": job_seeds, "J": J, "D": D, "lens": lens}


def judge_run(case, device, carry=True):
    """The calls through imitation.replay_judge on `device`; carry=False: every call starts from the plain loop's state in front of it (the
    kernel may hand the same positions to other envs than the loop does)."""
    from babyai_amd.imitation import replay_judge
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)
    first = case["calls"][0]["before"]
    job, pos, counters = t(first["job"].copy()), t(first["pos"].copy()), t(first["counters"].copy())
    res = {k: t(v.copy()) for k, v in first["results"].items()}
    n = len(first["job"])
    off, job_demo, job_seeds = t(case["offset"]), t(case["job_demo"]), t(case["job_seeds"].view(np.int64))
    ids, seeds = torch.full((n,), -7, dtype=torch.int64, device=device), torch.full((n,), -7, dtype=torch.int64, device=device)
    out = []
    for c in case["calls"]:
        if not carry:
            b = c["before"]
            job.copy_(t(b["job"])); pos.copy_(t(b["pos"])); counters.copy_(t(b["counters"]))
            for k in res:
                res[k].copy_(t(b["results"][k]))
        ids_before = ids.cpu().numpy().copy()
        replay_judge(t(c["fed"]), t(c["done"]), t(c["reward64"]), job, pos, off, res["played"], res["done_at"], res["return64"], c["claim"],
                     job_demo, job_seeds, ids, seeds, counters)
        out.append({"job": job.cpu().numpy().copy(), "pos": pos.cpu().numpy().copy(), "counters": counters.cpu().numpy().copy(),
                    "ids": ids.cpu().numpy().copy(), "seeds": seeds.cpu().numpy().view(np.uint64).copy(), "ids_before": ids_before,
                    "results": {k: v.cpu().numpy().copy() for k, v in res.items()}})
    return out


def assert_judge_equal(case, got):
    """Every field equal to the plain loop's (positions handed out in env order)."""
    for c, (g, w) in enumerate(zip(got, case["calls"])):
        for k in ("job", "pos", "counters"):
            assert np.array_equal(g[k], w[k]), (c, k, g[k], w[k])
        for k, v in w["results"].items():
            assert np.array_equal(g["results"][k].view(np.uint8), v.view(np.uint8)), (c, k)
        if w["claim"]:
            assert np.array_equal(g["ids"], w["ids"]), c
            got_seed = w["ids"] >= 0
            assert np.array_equal(g["seeds"][got_seed], w["seeds"][got_seed]), c
        else:
            assert np.array_equal(g["ids"], g["ids_before"]), c          # not touched
