#!/usr/bin/env python3
"""Fixtures of tests/golden/refpin/, recorded from the REFERENCE itself: babyai imported UNMODIFIED on the restated gym /
gym_minigrid shim of oracle/shim (oracle/refenv.py finds the tree; BABYAI_REFERENCE points elsewhere).  The reference tree never
travels with the repository: the fixtures are committed, and the tests replay the protocols of tests/refpin_util.py on the oracle
and on the engine's host build against them.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_refpin.py [part ...]      parts: levels random strict vocab rollout bot gen step (default: all)

  levels   the 105 registered ids, the constructor attributes of every level, and what the reference's own smoke test of
           levelgen.py reads (surface / grid of a seed-0 construction, the mission of its first reset)  -> levels.json
  random   tests/test_oracle_reference.py's random-action episodes of every level                      -> random_episodes.json
  strict   tests/test_strict_modes.py's episodes with the verifier's strict modes switched on           -> strict_modes.json
  vocab    the reference's InstructionsPreprocessor (babyai/utils/format.py) on tests/test_vocab_remap.py's missions -> vocab.npz
  rollout  the reference's BaseAlgo.collect_experiences (babyai/rl/algos/base.py) over tests/rollout_util.ToyACModel -> rollout.npz
  bot      the reference's expert (babyai/bot.py) answering tests/test_hostsim_bot.py's live protocols: every decision, step result
           and stack depth, in call order (refpin_util.Recording; the tests replay them)                 -> bot_reference.json.gz
  gen      the level digest (refpin_util.level_digest: grid, first observation, pose, max_steps, mission) of every registered level,
           seeds 52000 .. 52511, six consecutive resets each, over at most 8 worker processes         -> gen_digest/<Level>.npy, README.md
  step     the step digests (refpin_util.step_digest_stream): 256 streams of every registered level, seeds 53000 .. 53255, 128 or 320 steps of
           the reference's expert with 8 % random actions and auto-reset; the actions taken and a digest per 16-step block of every
           observation, direction, reward and done, over at most 8 worker processes                  -> step_digest/<Level>.npz, README.md
           (step-again: records once more into a scratch directory and writes into that README whether the bytes came out the same)
"""
import json
import os
import sys
import tempfile
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
from oracle import refenv  # noqa: E402
from oracle import levels as olevels  # noqa: E402
import refpin_util as rp  # noqa: E402

assert refenv.have_reference(), "needs the reference tree (BABYAI_REFERENCE)"
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    refenv.import_reference()
    from babyai.levels import level_dict  # noqa: E402


def write_json(name, obj):
    os.makedirs(rp.GOLDEN, exist_ok=True)
    with open(rp.golden_path(name), "w") as f:
        json.dump(obj, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", rp.golden_path(name))


def part_levels():
    attrs, smoke = {}, {}
    for name in sorted(level_dict):
        attrs[name] = rp.level_attrs(level_dict[name](seed=1))
        m0 = level_dict[name](seed=0)
        d = rp.Digest()
        d.add(m0.unwrapped.grid.encode(), np.uint8)
        rec = {"surface": m0.surface, "grid": d.hexdigest()}
        rec["reset_mission"] = m0.reset()["mission"]
        smoke[name] = rec
    write_json("levels.json", {"registered": sorted(level_dict), "attrs": attrs, "seed0": smoke})


def part_random():
    out = {}
    for name in sorted(olevels.SPECS):
        def env_for_seed(seed):
            e = rp.reference_level(level_dict, name)
            e.seed(seed)
            return e
        out[name] = rp.random_episodes(env_for_seed)
    write_json("random_episodes.json", out)


def part_strict():
    from babyai.levels.verifier import SeqInstr, AndInstr
    out = {}
    for name, leaf_bits, seq in rp.STRICT_CASES:
        def env_for_seed(seed):
            e = rp.reference_level(level_dict, name)
            e.seed(seed)
            return e

        def arm(ref):
            if seq and isinstance(ref.instrs, SeqInstr) and not isinstance(ref.instrs, AndInstr):
                ref.instrs.strict = True
            if leaf_bits:
                def leaves(i):
                    return leaves(i.instr_a) + leaves(i.instr_b) if isinstance(i, SeqInstr) else [i]
                for leaf in leaves(ref.instrs):
                    leaf.strict = True
        out[name] = rp.strict_episodes(env_for_seed, arm)
    write_json("strict_modes.json", out)


def part_vocab():
    from babyai.utils.format import InstructionsPreprocessor, get_vocab_path
    missions = rp.vocab_missions()
    with tempfile.TemporaryDirectory() as d:
        os.environ["BABYAI_STORAGE"] = d
        trained = InstructionsPreprocessor("trained")
        trained([{"mission": m} for m in missions[:300]])      # a "trained model": its vocabulary grew over the first 300 missions
        trained.vocab.save()
        vocab = json.load(open(get_vocab_path("trained")))
        ref = InstructionsPreprocessor("trained")                # ... continued from the saved file over all 10^4, 500 per batch
        rows = []
        for lo in range(0, len(missions), 500):
            rows += list(ref([{"mission": m} for m in missions[lo:lo + 500]]).numpy())
        width = max(len(r) for r in rows)
        ids = np.zeros((len(rows), width), dtype=np.int16)
        for i, r in enumerate(rows):
            ids[i, :len(r)] = r
        small = InstructionsPreprocessor("small")                # a vocabulary that has seen two missions
        small([{"mission": m} for m in missions[:2]])
        v2 = dict(small.vocab.vocab)
        known_only = [m for m in missions if all(w in v2 for w in m.replace(",", " ").split())][:200]
        again = InstructionsPreprocessor("small")
        again.vocab.vocab = dict(v2)
        again_rows = [list(again([{"mission": m}]).numpy()[0]) for m in known_only]
        w2 = max(len(r) for r in again_rows)
        again_ids = np.zeros((len(again_rows), w2), dtype=np.int16)
        for i, r in enumerate(again_rows):
            again_ids[i, :len(r)] = r
    os.makedirs(rp.GOLDEN, exist_ok=True)
    np.savez_compressed(rp.golden_path("vocab.npz"), missions_sha256=rp.missions_digest(missions), trained_vocab=json.dumps(vocab, sort_keys=True),
                        ids=ids, small_vocab=json.dumps(v2, sort_keys=True), known_only=np.array(known_only), again_ids=again_ids)
    print("wrote", rp.golden_path("vocab.npz"))


def part_rollout():
    import gym
    import torch
    from babyai.rl.algos.base import BaseAlgo
    from babyai.rl.utils import DictList
    from rollout_util import ToyACModel, pad_tokens

    class Algo(BaseAlgo):
        def update_parameters(self):
            pass

    def preprocess(obss, device=None):
        return DictList({"image": torch.tensor(np.array([o["image"] for o in obss]), dtype=torch.float),
                         "instr": torch.tensor(pad_tokens([o["mission"] for o in obss]))})

    out = {}
    for level, scale in rp.ROLLOUT_CASES:
        envs = []
        for s in rp.ROLLOUT_SEEDS:
            e = gym.make("BabyAI-%s-v0" % level)
            e.seed(int(s))
            envs.append(e)
        algo = Algo(envs, ToyACModel(), rp.ROLLOUT_T, 0.99, 7e-4, 0.95, 0.01, 0.5, 0.5, 1, preprocess,
                    lambda _0, _1, reward, _2, scale=scale: scale * reward, None)
        for it in range(rp.ROLLOUT_ITERS):                   # state carries across rollouts (memory, masks, log tails)
            exps, log = algo.collect_experiences()
            for f in rp.ROLLOUT_FIELDS + ("obs.image", "obs.instr"):
                t = getattr(exps.obs, f[4:]) if f.startswith("obs.") else getattr(exps, f)
                out[rp.rollout_key(level, scale, it, f)] = t.numpy()
            for k in ("num_frames", "episodes_done"):
                out[rp.rollout_key(level, scale, it, k)] = np.array(log[k])
            for k in ("num_frames_per_episode", "return_per_episode", "reshaped_return_per_episode"):
                out[rp.rollout_key(level, scale, it, k)] = np.array(log[k], dtype=np.float64 if "return" in k else np.int64)
        del algo                                             # (ParallelEnv.__del__ ends its worker processes)
    os.makedirs(rp.GOLDEN, exist_ok=True)
    np.savez_compressed(rp.golden_path("rollout.npz"), **out)
    print("wrote", rp.golden_path("rollout.npz"))


def part_bot():
    import test_hostsim_bot as tb
    out = {}

    def record(key, protocol, *args):
        rec = rp.Recording(rp.LiveBotRef())
        protocol(rec, *args)                                 # (the host build is checked against the live answers as they come)
        out[key] = rec.log
    for level, n_envs, steps in tb.DIFFERENTIAL:
        record("differential/%s" % level, tb._differential, level, n_envs, steps)
    for level in tb.SWITCH_ON:
        record("switch_on/%s" % level, tb._switch_on, level)
    record("stack_capacity", tb._stack_capacity)
    os.makedirs(rp.GOLDEN, exist_ok=True)
    import gzip
    with gzip.GzipFile(rp.golden_path("bot_reference.json.gz"), "wb", mtime=0) as f:     # (mtime 0: the same bytes on every run)
        f.write((json.dumps(out, sort_keys=True, separators=(",", ":")) + "\n").encode())
    print("wrote", rp.golden_path("bot_reference.json.gz"))


def _gen_kind(name):
    """uint32[512, 6]: the reference's digests of one kind -- Level(), .seed(52000 + i), six reset()s in a row."""
    out = np.zeros((rp.GEN_DIGEST_SEEDS, rp.GEN_DIGEST_LEVELS), np.uint32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(rp.GEN_DIGEST_SEEDS):
            env = rp.reference_level(level_dict, name)
            env.seed(rp.GEN_DIGEST_SEED0 + i)
            for k in range(rp.GEN_DIGEST_LEVELS):
                obs = env.reset()
                out[i, k] = rp.env_level_digest(env, obs)
    return name, out


def part_gen():
    import multiprocessing
    names = sorted(level_dict)
    d = rp.golden_path("gen_digest")
    os.makedirs(d, exist_ok=True)
    with multiprocessing.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        got = dict(pool.imap_unordered(_gen_kind, names))
    lines = ["# Level digests of the reference's generator", "",
             "`<Level>.npy` = `uint32[%d, %d]`: `refpin_util.level_digest` (grid after the reset, first observation, agent pose, `max_steps`,"
             % (rp.GEN_DIGEST_SEEDS, rp.GEN_DIGEST_LEVELS),
             "mission) of the reference's level object after `.seed(%d + i)` and each of six `reset()` calls in a row.  Recorded from the"
             % rp.GEN_DIGEST_SEED0,
             "reference itself, never edited by hand; regenerate (byte-identical) where the reference tree can be imported with", "",
             "    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_refpin.py gen", "",
             "Distinct digests among the %d of each kind (a kind with few objects and a small room repeats levels; a digest that"
             % (rp.GEN_DIGEST_SEEDS * rp.GEN_DIGEST_LEVELS),
             "saw less than the whole level would repeat far more often):", "", "| level | distinct |", "|---|---|"]
    for name in names:
        np.save(os.path.join(d, name + ".npy"), got[name])
        distinct = len(np.unique(got[name]))
        print("%-28s %4d distinct of %d" % (name, distinct, got[name].size))
        lines.append("| %s | %d |" % (name, distinct))
    with open(os.path.join(d, "README.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", d)


# ---- step: the step digests --------------------------------------------------------------------------------------------------
STEP_CHUNK = 32                     # streams per task: 8 tasks per kind, so that the long kinds spread over the workers
# kinds allowed fewer than 100 successful episodes, each with its reason
STEP_FEW_SUCCESSES = {
    "KeyInBox": "the key is in a box, and the reference's expert opens no box: it raises at the first decision of every episode; a longer T of random actions solves no more",
}


def _step_task(task):
    import time
    from babyai.bot import Bot
    name, lo = task
    t0 = time.time()
    steps = rp.step_digest_steps(name)
    policies = {}

    def env_for_seed(seed):
        e = rp.reference_level(level_dict, name)
        e.seed(seed)
        return e

    def policy_for_stream(i):
        policies[i] = rp.ExpertPolicy(Bot, rp.STEP_DIGEST_SEED0 + i)
        return policies[i]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = rp.step_digest_run(env_for_seed, range(lo, lo + STEP_CHUNK), steps, policy_for_stream)
    out["budget"] = np.array([(t, i) for i in sorted(policies) for t in policies[i].budget], np.int32).reshape(-1, 2)
    return name, lo, out, time.time() - t0


def _step_record(out_dir, only=None):
    """Records every kind (only: these) into out_dir/<Level>.npz -> {kind: statistics}, the wall time of the recording and the kinds refused."""
    import multiprocessing
    import time
    names = sorted(level_dict)
    assert names == sorted(olevels.SPECS)
    names = [n for n in names if only is None or n in only]
    refused = []
    tasks = [(n, lo) for n in names for lo in range(0, rp.STEP_DIGEST_STREAMS, STEP_CHUNK)]
    tasks.sort(key=lambda t: -rp.step_digest_steps(t[0]))            # the long ones first
    limit = max(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(os.path.dirname(rp.GOLDEN)) for f in fs if "step_digest" not in d)
    os.makedirs(out_dir, exist_ok=True)
    t0 = time.time()
    parts, stats = {}, {}
    with multiprocessing.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        for name, lo, out, secs in pool.imap_unordered(_step_task, tasks):
            parts.setdefault(name, {})[lo] = (out, secs)
            if len(parts[name]) * STEP_CHUNK == rp.STEP_DIGEST_STREAMS:
                chunks = [parts[name][k][0] for k in sorted(parts[name])]
                o = {k: np.concatenate([c[k] for c in chunks], axis=0 if k in ("first_image", "first_direction", "ends", "budget") else 1)
                     for k in chunks[0]}
                dead, done = o["bot_dead"], o["done"] != 0
                rising = dead.copy()
                rising[1:] &= ~dead[:-1] | done[:-1]
                st = {"steps": int(dead.shape[0]), "success": int(o["ends"][:, 0].sum()), "failure": int(o["ends"][:, 1].sum()),
                      "timeout": int(o["ends"][:, 2].sum()), "dead": int(rising.sum()), "budget": int(len(o["budget"])),
                      "suggested": int(o["suggested"].sum()), "cpu_s": sum(parts[name][k][1] for k in parts[name])}
                if st["success"] < 100 and name not in STEP_FEW_SUCCESSES:
                    refused.append("%s: %d successful episodes, fewer than 100: raise its T" % (name, st["success"]))
                    print("NOT WRITTEN", refused[-1], flush=True)
                    del parts[name]
                    continue
                path = os.path.join(out_dir, name + ".npz")
                np.savez_compressed(path, actions=rp.pack_actions(o["action"]), first=rp.step_first_digests(o["first_image"], o["first_direction"]),
                                    digest=rp.step_block_digests(o["image"], o["direction"], o["reward"], o["done"]),
                                    suggested=rp.pack_bits(o["suggested"]), bot_dead=rp.pack_bits(o["bot_dead"]), budget=o["budget"],
                                    ends=o["ends"])
                st["bytes"] = os.path.getsize(path)
                assert st["bytes"] <= limit, "%s: %d bytes, more than the largest golden file (%d): lower its T" % (name, st["bytes"], limit)
                stats[name] = st
                del parts[name]
                print("%-28s T %3d  success %5d failure %4d timeout %4d  dead %4d (budget %3d)  %6d bytes  %6.1f cpu-s"
                      % (name, st["steps"], st["success"], st["failure"], st["timeout"], st["dead"], st["budget"], st["bytes"], st["cpu_s"]), flush=True)
    return stats, time.time() - t0, refused


def _step_readme(d, stats, wall, second):
    lines = ["# Step digests of the reference's episodes", "",
             "`<Level>.npz`, recorded from the reference itself (never edited by hand) by", "",
             "    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_refpin.py step", "",
             "Per kind %d streams, stream i seeded %d + i, stepped T times with auto-reset (tests/refpin_util.py step_digest_stream) under a"
             % (rp.STEP_DIGEST_STREAMS, rp.STEP_DIGEST_SEED0),
             "closed-loop policy: the reference's expert, a fresh one per episode, overridden with probability %g by a uniform random action; every"
             % rp.STEP_DIGEST_OVERRIDE,
             "decision under a budget of %g s; an expert that raised or ran out of budget is dead for the rest of its episode, which goes on"
             % rp.STEP_DIGEST_BUDGET_S,
             "with random actions (refpin_util.ExpertPolicy).  T = 128 in one room, 320 in several; raised for "
             + ", ".join("%s (%d)" % kv for kv in sorted(rp.STEP_DIGEST_LONGER.items())) + ", which had fewer than 100 successes at 320.", "",
             "- `actions` uint8[T, S / 2]: two actions per byte (stream 2k low, 2k + 1 high);",
             "- `digest` uint32[S, T / 16]: per 16-step block the first 4 bytes of sha256, little endian, over every step's image uint8[7, 7, 3],",
             "  direction (1 byte), reward (float64) and done (1 byte); `first` uint32[S]: the same of the first observation and direction;",
             "- `suggested`, `bot_dead` uint8[T, S / 8]: one bit per (t, i) (numpy packbits): the action is the expert's own suggestion / the expert was dead;",
             "- `budget` int32[k, 2]: the (t, i) at which an expert died of the budget, not of an exception; `ends` int64[S, 3]: episodes ended by success,",
             "  by failure before the time limit, by the time limit.", "",
             "Recording time: %.0f s wall over %d worker processes (%.0f s in the workers; %d steps, %.0f steps per second per worker)."
             % (wall, min(8, os.cpu_count() or 1), sum(s["cpu_s"] for s in stats.values()),
                sum(s["steps"] for s in stats.values()) * rp.STEP_DIGEST_STREAMS,
                sum(s["steps"] for s in stats.values()) * rp.STEP_DIGEST_STREAMS / sum(s["cpu_s"] for s in stats.values())), "",
             "Kinds allowed fewer than 100 successes: " + "; ".join("%s (%s)" % kv for kv in sorted(STEP_FEW_SUCCESSES.items())) + ".", "",
             "| level | T | success | failure | time limit | dead-expert episodes | of them by budget | expert's own actions | bytes | cpu-s |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for name in sorted(stats):
        s = stats[name]
        lines.append("| %s | %d | %d | %d | %d | %d | %d | %d | %d | %.0f |" % (name, s["steps"], s["success"], s["failure"], s["timeout"], s["dead"],
                                                                           s["budget"], s["suggested"], s["bytes"], s["cpu_s"]))
    tot = {k: sum(s[k] for s in stats.values()) for k in ("success", "failure", "timeout", "dead", "budget", "suggested", "bytes")}
    lines.append("| total | | %d | %d | %d | %d | %d | %d | %d | |" % (tot["success"], tot["failure"], tot["timeout"], tot["dead"], tot["budget"],
                                                                   tot["suggested"], tot["bytes"]))
    lines += ["", SECOND_MARK, "", second]
    with open(os.path.join(d, "README.md"), "w") as f:
        f.write("\n".join(lines) + "\n")


SECOND_MARK = "## Second recording"


def part_step():
    """BBAI_STEP_DIGEST_KINDS=A,B records those kinds only and keeps the others' files and statistics (recording.json)."""
    d = rp.golden_path("step_digest")
    only = os.environ.get("BBAI_STEP_DIGEST_KINDS")
    stats, wall, refused = _step_record(d, only.split(",") if only else None)
    log = os.path.join(d, "recording.json")
    if only:
        with open(log) as f:
            old = json.load(f)
        stats, wall = dict(old["kinds"], **stats), old["wall_s"] + wall
    with open(log, "w") as f:
        json.dump({"kinds": stats, "wall_s": wall}, f, indent=0, sort_keys=True)
        f.write("\n")
    _step_readme(d, stats, wall, "Not made yet: `python tools/gen_golden_refpin.py step-again` records once more and compares.")
    print("wrote %s in %.0f s" % (d, wall))
    if refused:
        raise SystemExit("\n".join(refused))


def part_step_again():
    """Records a second time into a scratch directory, compares file by file with the committed recording and writes the outcome into its README."""
    d = rp.golden_path("step_digest")
    with tempfile.TemporaryDirectory() as tmp:
        stats, wall, refused = _step_record(tmp)
        assert not refused, refused
        differ = []
        for name in sorted(stats):
            with open(os.path.join(tmp, name + ".npz"), "rb") as a, open(os.path.join(d, name + ".npz"), "rb") as b:
                if a.read() != b.read():
                    with np.load(os.path.join(d, name + ".npz")) as z:
                        differ.append("%s (budget deaths: %d in the committed recording, %d in the second)" % (name, len(z["budget"]), stats[name]["budget"]))
    second = ("A second recording (%.0f s wall) gave %d of %d files byte-identical to the committed ones." % (wall, len(stats) - len(differ), len(stats))
              + ("  Different: " + "; ".join(differ) + "." if differ else ""))
    readme = os.path.join(d, "README.md")
    with open(readme) as f:
        text = f.read()
    with open(readme, "w") as f:
        f.write(text[:text.index(SECOND_MARK)] + SECOND_MARK + "\n\n" + second + "\n")
    print(second)


PARTS = {"levels": part_levels, "random": part_random, "strict": part_strict, "vocab": part_vocab, "rollout": part_rollout, "bot": part_bot, "gen": part_gen,
         "step": part_step, "step-again": part_step_again}

if __name__ == "__main__":
    for p in sys.argv[1:] or [p for p in PARTS if p != "step-again"]:
        PARTS[p]()
