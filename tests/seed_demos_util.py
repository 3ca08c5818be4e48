"""Helpers of tests/test_seed_demos_host.py and tests/test_gpu_seed_demos.py: the host build behind the tensor protocol that
`DemoStore.collect_seeds(env=...)` drives (HostPool), the per-seed episodes it must reproduce (HostEnv + HostBot, one env, one seed, no pool),
synthetic chunks with a plain Python loop for `demo_jobs`, and synthetic rings with direct indexing for `demo_pack_list`.  Everything is
computed once per process (lru_cache), shared by the tests and never written to."""
import functools
import hashlib
import os

import numpy as np
import torch

from babyai_amd import missions
from babyai_amd.levels import make_cfg
from hostsim_util import HostBatch, HostBot, HostEnv
from scenario_util import ScenarioModel

TOK_MAX = 72
ROW = 147
GOLDEN_DEMOS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "demos", "bot_demos.npz")
# (level, seeds, pool, chunk, kept, frames or None): the cases of the issue, every expected value recomputed by the tests
CASES = {"PickupDist": ("PickupDist", (1000, 1300), 37, 4, 281, 1416), "UnlockToUnlock": ("UnlockToUnlock", (1000, 1060), 9, 16, 34, None),
         "BossLevel": ("BossLevel", (1000, 1040), 7, 16, 40, 3555)}
GOLDEN_LEVELS = ("GoToLocal", "PutNextLocal", "PickupDist", "BossLevel", "UnlockToUnlock")
GOLDEN_DROPPED = {"PickupDist": [332, 372, 375, 376], "UnlockToUnlock": [10]}


def steps_bound(cfg):
    return 8 * cfg.room_size ** 2 * cfg.num_rows * cfg.num_cols


# ---- the host build behind collect_seeds' env protocol --------------------------------------------------------------------------------
class HostPool(object):
    """ScenarioModel (hostsim_util.HostBatch + the host build of the expert) as the `env=` of collect_seeds: CPU tensors in and out."""

    def __init__(self, level, seeds, done_actions=False):
        self.model = ScenarioModel(level, np.asarray(seeds, dtype=np.uint64), auto_reset=True)
        self.done_actions = bool(done_actions)
        if done_actions:                        # the reference's BABYAI_DONE_ACTIONS mode, the expert's `done` counting as the enum member (bbai_bot_rollout)
            self.model.hb = HostBatch(self.model.cfg, np.asarray(seeds, dtype=np.uint64), auto_reset=True, done_actions=True, enum_done=True)
            self.model.hb.reset()
        self.num_envs, self.device = self.model.n, torch.device("cpu")
        self.max_steps_bound = steps_bound(self.model.cfg)
        self.rollouts = self.reseeds = 0
        self.closed = False

    def bot_rollout(self, steps, tokens=False, out=None):
        m, hb = self.model, self.model.hb
        assert tokens and out is not None
        o = {k: v.numpy() for k, v in out.items()}
        assert o["image"].shape == (steps, m.n, 7, 7, 3)
        for t in range(steps):
            o["image"][t], o["direction"][t], o["tokens"][t] = hb.image, hb.direction, m.tokens()
            act, gave = m.bot_decide()
            m.step(act)
            o["action"][t], o["gave_up"][t], o["reward"][t], o["done"][t] = act, gave, hb.reward, hb.done
        self.rollouts += 1
        return out

    def reseed(self, ids, seeds):
        self.model.reseed(ids.numpy(), seeds.numpy().view(np.uint64))
        if self.done_actions:                   # a new episode: lastStepMatch cleared
            listed = ids.numpy()
            self.model.hb.lsm[listed[(listed >= 0) & (listed < self.num_envs)]] = 0
        self.reseeds += 1

    def close(self):
        self.closed = True


# ---- one seed, one env, one episode: what train_intelligent_expert.py:106-147 does per listed seed --------------------------------------
@functools.lru_cache(maxsize=None)
def seed_episode(level, seed):
    """(kept, token row, images uint8[L, 7, 7, 3], directions uint8[L], actions uint8[L]) of the episode env.seed(seed); env.reset() starts."""
    env = HostEnv(make_cfg(level), seed)
    img = env.reset()
    bot = HostBot(env)
    ids = missions.tokenize(env.mission)[:TOK_MAX]
    tok = np.zeros(TOK_MAX, np.uint8)
    tok[:len(ids)] = ids
    images, dirs, acts = [], [], []
    first = True
    while True:
        a = bot.decide(first)
        first = False
        if a is None:                           # a bot exception: the seed is skipped (:141-143)
            return False, tok, None, None, None
        images.append(img)
        dirs.append(env.agent[2])
        acts.append(a)
        img, reward, done = env.step(a)
        if done:
            break
    out = (bool(reward > 0), tok, np.stack(images), np.array(dirs, np.uint8), np.array(acts, np.uint8))
    for a in out[1:]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(level, seeds):
    """The store fields collect_seeds must return for `seeds` (a tuple): dict of numpy arrays + kept."""
    eps = [seed_episode(level, int(s)) for s in seeds]
    kept = np.array([j for j, e in enumerate(eps) if e[0]], dtype=np.int64)
    lens = [len(eps[j][4]) for j in kept]
    cat = lambda i, shape: np.concatenate([eps[j][i] for j in kept]) if len(kept) else np.zeros(shape, np.uint8)
    out = {"kept": kept, "image": cat(2, (0, 7, 7, 3)), "direction": cat(3, (0,)), "action": cat(4, (0,)),
           "tokens": np.stack([eps[j][1] for j in kept]) if len(kept) else np.zeros((0, TOK_MAX), np.uint8),
           "offset": np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), "gave_up": sum(1 for e in eps if e[2] is None)}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def assert_store_is(store, kept, want):
    assert np.array_equal(np.asarray(kept), want["kept"]), (kept, want["kept"])
    assert np.asarray(kept).dtype == np.int64
    assert len(store) == len(want["kept"]) and store.num_frames == int(want["offset"][-1])
    assert np.array_equal(store.offset_host, want["offset"]) and np.array_equal(store.offset.cpu().numpy(), want["offset"])
    for k in ("image", "direction", "action", "tokens"):
        got = getattr(store, k).cpu().numpy()
        assert got.shape == want[k].shape and np.array_equal(got, want[k]), k


@functools.lru_cache(maxsize=None)
def golden(level):
    with np.load(GOLDEN_DEMOS) as f:
        g = {k[len(level) + 1:]: f[k] for k in f.files if k.startswith(level + "_")}
    g["ends"] = np.cumsum(g["length"])
    return g


def assert_kept_equal_golden(level, store, kept):
    """Every kept demo k of seeds seed + arange(n) equals demo k recorded from the reference's own script."""
    g = golden(level)
    img, dirs, acts, off = store.image.cpu().numpy(), store.direction.cpu().numpy(), store.action.cpu().numpy(), store.offset_host
    text = store.to_reference()
    for d, k in enumerate(np.asarray(kept).tolist()):
        lo, hi = int(g["ends"][k] - g["length"][k]), int(g["ends"][k])
        a, b = int(off[d]), int(off[d + 1])
        assert text[d][0] == str(g["mission"][k]), (level, k)
        assert acts[a:b].tolist() == g["actions"][lo:hi].tolist(), (level, k)
        assert dirs[a:b].tolist() == g["directions"][lo:hi].tolist(), (level, k)
        assert hashlib.sha256(np.ascontiguousarray(img[a:b]).tobytes()).hexdigest() == str(g["image_sha"][k]), (level, k)


def golden_seeds(level):
    g = golden(level)
    return tuple(int(g["seed"]) + k for k in range(len(g["length"])))


# ---- synthetic chunks for demo_jobs ---------------------------------------------------------------------------------------------------
JOBS_CASES = [(n, chunk, p) for n in (1, 63, 64, 65, 200) for chunk in (1, 4, 16) for p in (0.02, 0.3)]


@functools.lru_cache(maxsize=None)
def jobs_case(n, chunk, p_done, calls=4):
    """`calls` chunks in a row for a pool of n envs (some idle from the start), with done on a chunk's first and last row, gave_up rows,
    reward == 0 rows, and a job list sized by what the plain loop finds so that it runs out in the middle of the last call but one."""
    rng = np.random.default_rng(1000 * n + 10 * chunk + int(p_done * 100))
    idle = rng.random(n) < 0.1
    idle[rng.integers(0, n)] = False
    if n > 1:
        idle[(int(np.flatnonzero(~idle)[0]) + 1) % n] = True
    live_ids = np.flatnonzero(~idle)
    live = len(live_ids)
    job0 = np.full(n, -1, dtype=np.int32)
    job0[live_ids] = np.arange(live, dtype=np.int32)
    chunks = []
    for c in range(calls):
        done = (rng.random((chunk, n)) < p_done).astype(np.uint8)
        gave = (done != 0) & (rng.random((chunk, n)) < 0.2)
        reward = np.where(rng.random((chunk, n)) < 0.25, 0.0, rng.random((chunk, n)) * 0.9 + 0.05).astype(np.float32)
        pick = rng.permutation(live_ids)[:4]                     # four envs in play whose columns are set by hand (fewer in a tiny pool)
        done[:, pick] = 0
        gave[:, pick] = False
        done[0, pick[0]] = 1                                     # done on the chunk's first row: kept
        reward[0, pick[0]] = 0.5
        if len(pick) == 4:
            done[chunk - 1, pick[1]] = 1                         # ... on its last row: kept
            reward[chunk - 1, pick[1]] = 0.25
            done[chunk // 2, pick[2]] = 1                        # the expert gave up
            gave[chunk // 2, pick[2]] = True
            done[chunk - 1, pick[3]] = 1                         # a failed mission: reward == 0
            reward[chunk - 1, pick[3]] = 0.0
        reward[gave] = 0.0
        chunks.append({"done": done, "gave_up": gave.astype(np.uint8), "reward": reward})
    # the finishes of the first calls with an endless list: the list ends inside call `calls - 2` if that call has more than one finish
    endless = jobs_run_reference(chunks, chunk, job0, np.arange(1 << 20, dtype=np.uint64), live)
    upto = [int(r["counters"][1]) for r in endless]
    before, inside = (upto[calls - 3] if calls >= 3 else 0), upto[calls - 2]
    J = live + before + max(0, (inside - before) // 2)
    seeds = rng.integers(0, 1 << 63, size=max(J, 1), dtype=np.uint64)[:J] if J else np.zeros(0, np.uint64)
    want = jobs_run_reference(chunks, chunk, job0, seeds, live)
    job0.setflags(write=False)
    return {"chunks": chunks, "job0": job0, "seeds": seeds, "cursor0": live, "want": want, "J": J}


def jobs_run_reference(chunks, chunk, job0, seeds, cursor0):
    """demo_jobs as a plain Python loop over envs and rows, call after call; the state after every call."""
    n, J = len(job0), len(seeds)
    job, start = job0.copy(), np.zeros(n, np.int32)
    cursor, finished, out = cursor0, 0, []
    for c, ch in enumerate(chunks):
        g0 = c * chunk
        ids, sd, rec, fin = np.full(n, -1, np.int64), np.zeros(n, np.uint64), [], np.zeros(n, bool)
        for i in range(n):
            if job[i] < 0:
                continue
            for t in range(chunk):
                if ch["done"][t, i]:
                    fin[i] = True
                    if ch["gave_up"][t, i] == 0 and ch["reward"][t, i] > 0:
                        rec.append((i, int(start[i]), g0 + t - int(start[i]) + 1, int(job[i])))
                    finished += 1
                    if cursor < J:
                        ids[i], sd[i], job[i], start[i] = i, seeds[cursor], cursor, g0 + chunk
                    else:
                        job[i] = -1
                    cursor += 1
                    break
        out.append({"ids": ids, "seeds": sd, "rec": np.array(rec, np.int32).reshape(-1, 4), "fin": fin, "job": job.copy(), "start": start.copy(),
                    "counters": np.array([cursor, finished, len(rec), sum(r[2] for r in rec)], np.int64)})
    return out


def jobs_run(case, chunk, device, carry=True):
    """The same calls through imitation.demo_jobs on `device`; the state after every call, as numpy.  carry=False: every call starts from the
    plain loop's state in front of it instead of from what the previous call left (the kernel may hand the same jobs to other envs than the
    loop does, and the calls behind that are then not comparable env by env)."""
    from babyai_amd.imitation import demo_jobs
    n = len(case["job0"])
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)
    job, start = t(case["job0"].copy()), torch.zeros(n, dtype=torch.int32, device=device)
    seeds = t(case["seeds"].view(np.int64))
    ids, sd = torch.full((n,), -7, dtype=torch.int64, device=device), torch.zeros(n, dtype=torch.int64, device=device)
    rec = torch.zeros((n, 4), dtype=torch.int32, device=device)
    counters = t(np.array([case["cursor0"], 0, 0, 0], np.int64))
    out = []
    for c, ch in enumerate(case["chunks"]):
        if not carry and c:
            w = case["want"][c - 1]
            job.copy_(t(w["job"]))
            start.copy_(t(w["start"]))
            counters.copy_(t(w["counters"]))
        job_before = job.cpu().numpy().copy()
        demo_jobs(t(ch["done"]), t(ch["gave_up"]), t(ch["reward"]), c * chunk, job, start, seeds, ids, sd, rec, counters)
        cn = counters.cpu().numpy().copy()
        out.append({"ids": ids.cpu().numpy().copy(), "seeds": sd.cpu().numpy().view(np.uint64).copy(), "rec": rec.cpu().numpy()[:int(cn[2])].copy(),
                    "job": job.cpu().numpy().copy(), "start": start.cpu().numpy().copy(), "counters": cn, "job_before": job_before})
    return out


# ---- synthetic rings for demo_pack_list ------------------------------------------------------------------------------------------------
class ListCase(object):
    """A ring of R slots of T steps of n streams of random bytes, `count` records, and what demo_pack_list must make of them (direct
    indexing).  first steps lie up to several ring turns in, so slots are addressed modulo R."""

    def __init__(self, seed, R, T, n, lens, aligned_long=True):
        rng = np.random.default_rng(seed)
        lens = np.asarray(lens, dtype=np.int64)
        count = len(lens)
        assert lens.min() >= 1 and lens.max() <= R * T
        self.R, self.T, self.n = R, T, n
        self.ring = [{"image": rng.integers(0, 256, (T, n, 7, 7, 3), dtype=np.uint8), "direction": rng.integers(0, 256, (T, n), dtype=np.uint8),
                      "action": rng.integers(0, 256, (T, n), dtype=np.uint8), "tokens": rng.integers(0, 256, (T, n, TOK_MAX), dtype=np.uint8),
                      "done": np.zeros((T, n), np.uint8)} for _ in range(R)]
        first = rng.integers(0, 5 * R * T, size=count)
        full = lens > (R - 1) * T                # a demo longer than R - 1 slots must start on a slot's first row to fit the ring
        first[full] = first[full] // T * T
        self.rec = np.stack([rng.integers(0, n, size=count), first, lens, rng.permutation(count)], axis=1).astype(np.int32)
        self.offset = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.frames = int(self.offset[-1])
        image, direction = np.zeros((self.frames, 7, 7, 3), np.uint8), np.zeros(self.frames, np.uint8)
        action, tokens = np.zeros(self.frames, np.uint8), np.zeros((count, TOK_MAX), np.uint8)
        phases = set()
        for k in range(count):
            s = int(self.rec[k, 0])
            for i in range(int(lens[k])):
                g = int(first[k]) + i
                slot, row = self.ring[(g // T) % R], g % T
                image[self.offset[k] + i], direction[self.offset[k] + i], action[self.offset[k] + i] = slot["image"][row, s], slot["direction"][row, s], slot["action"][row, s]
                phases.add(((row * n + s) * ROW) % 16)
            g = int(first[k])
            tokens[k] = self.ring[(g // T) % R]["tokens"][g % T, s]
        self.phases = phases                    # byte phases of the source rows relative to their (16-byte aligned) arrays
        self.slots_spanned = (first + lens - 1) // T - first // T + 1
        self.wraps = bool(((first // T) % R + self.slots_spanned > R).any())
        self.expect = {"image": image, "direction": direction, "action": action, "tokens": tokens}
        for a in self.expect.values():
            a.setflags(write=False)

    def run(self, device):
        from babyai_amd.imitation import demo_pack_list
        ring = [{k: torch.as_tensor(v, device=device) for k, v in slot.items()} for slot in self.ring]
        store = demo_pack_list(ring, self.T, torch.as_tensor(self.rec, device=device), self.frames)
        return store

    def check(self, store):
        assert len(store) == len(self.rec) and store.num_frames == self.frames
        assert np.array_equal(store.offset.cpu().numpy(), self.offset) and np.array_equal(store.offset_host, self.offset)
        for k, want in self.expect.items():
            got = getattr(store, k).cpu().numpy()
            assert got.shape == want.shape and np.array_equal(got, want), k
