#!/usr/bin/env python3
"""Fixtures of tests/golden/imitation/, recorded from the REFERENCE itself (babyai imported UNMODIFIED on the shim of oracle/shim,
like tools/gen_golden_refpin.py; build container only -- the reference tree never travels with the repository).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_imitation.py

  demos_<level>.npz   a dozen demonstrations per level of tests/imitation_util.LEVELS, made by the reference's expert in the loop of
                      scripts/make_agent_demos.py:71-137, images stored plainly
  cases.npz           the reference's `ImitationLearning.run_epoch_recurrence_one_batch` (babyai/imitation.py:225-321, with its own
                      `transform_demos` and `ObssPreprocessor`) over tests/imitation_util.ToyILModel: per case every model call's inputs, the
                      returned log and the parameters after one SGD step, all from the reference; the batch's sorted order, inds, mask,
                      episode_ids and action_true restated by this tool (locals of the reference's function: the recorded calls pin
                      them); and `run_epoch_recurrence` in validation mode: its log
  vocab.json          the reference Vocabulary those runs grew (first-seen order)

Every case keeps its means over a power of two of frames (see imitation_util): the tool picks the demos accordingly and repeats each
case in float64 to prove that nothing was rounded.
"""
import itertools
import json
import os
import sys
import tempfile
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True
from oracle import refenv  # noqa: E402
import imitation_util as iu  # noqa: E402

assert refenv.have_reference(), "needs the reference tree (BABYAI_REFERENCE)"
os.environ["BABYAI_STORAGE"] = tempfile.mkdtemp()
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    refenv.import_reference()
    import torch  # noqa: E402
    import blosc  # noqa: E402
    from babyai.levels import level_dict  # noqa: E402
    from babyai.bot import Bot  # noqa: E402
    from babyai.imitation import ImitationLearning  # noqa: E402
    from babyai.utils.format import ObssPreprocessor  # noqa: E402

N_DEMOS, SEED = 12, 500


def record_demos(level):
    """scripts/make_agent_demos.py:71-137 with BotAgent: demo k = the first episode of stream SEED + k the bot solves."""
    env = level_dict[level]()
    demos, crashed = [], False
    while len(demos) < N_DEMOS:
        if not crashed:
            env.seed(SEED + len(demos))
        obs = env.reset()
        bot = Bot(env)
        mission, images, directions, actions = obs["mission"], [], [], []
        done, reward = False, 0
        try:
            while not done:
                action = int(bot.replan())
                new_obs, reward, done, _ = env.step(action)
                actions.append(action)
                images.append(obs["image"])
                directions.append(obs["direction"])
                obs = new_obs
        except Exception:
            crashed = True
            continue
        crashed = reward == 0
        if reward > 0:
            demos.append((mission, np.array(images, dtype=np.uint8), directions, actions))
    os.makedirs(iu.GOLDEN, exist_ok=True)
    np.savez_compressed(os.path.join(iu.GOLDEN, "demos_%s.npz" % level), mission=np.array([d[0] for d in demos]).astype(str),
                        length=np.array([len(d[3]) for d in demos], np.int32), image=np.concatenate([d[1] for d in demos]),
                        direction=np.concatenate([np.array(d[2], np.uint8) for d in demos]), action=np.concatenate([np.array(d[3], np.uint8) for d in demos]))
    return demos


def pow2(x):
    return x >= 1 and x & (x - 1) == 0


def pick(lengths, want, recurrence, divides, repeat=False):
    """`want` demo numbers whose frame count F has floor(F / recurrence) a power of two, and recurrence | F or not as asked; with
    `repeat`, the first one appears twice and some other demo shares its length (the sort must be stable)."""
    for combo in itertools.permutations(range(len(lengths)), want):
        idx = list(combo) + ([combo[0]] if repeat else [])
        F = int(sum(lengths[i] for i in idx))
        if pow2(F // recurrence) and (F % recurrence == 0) == divides:
            if not repeat or len(set(lengths[i] for i in idx)) < len(idx) - 1:
                return idx
    raise SystemExit("no such batch among the recorded demos")


def learner(model, preproc, recurrence, batch_size=4):
    il = ImitationLearning.__new__(ImitationLearning)                  # (its __init__ builds envs, a model and a storage directory)
    il.acmodel, il.obss_preprocessor, il.device = model, preproc, torch.device("cpu")
    il.args = types.SimpleNamespace(recurrence=recurrence, entropy_coef=iu.ENTROPY_COEF, batch_size=batch_size)
    il.optimizer = torch.optim.SGD(model.parameters(), lr=iu.LR)
    return il


def reference_structures(batch):
    """What imitation.py:226-251 builds before the first model call.  These are locals of the reference's function, so they are
    RESTATED here (Python's own stable sort, a prefix sum), not recorded from it; what pins them to the reference is the recorded
    model calls, whose rows the reference picks with exactly these structures."""
    order = sorted(range(len(batch)), key=lambda i: len(batch[i][3]), reverse=True)       # Python's stable sort, as batch.sort(key=len, reverse=True)
    lens = [len(batch[i][3]) for i in order]
    inds = np.concatenate([[0], np.cumsum(lens)])[:-1]
    return order, lens, inds


def main():
    out, demos = {}, {}
    for level in iu.LEVELS:
        demos[level] = record_demos(level)
        print(level, "lengths", [len(d[3]) for d in demos[level]])
    preproc = ObssPreprocessor("golden_imitation")
    packed = {lv: [(d[0], blosc.pack_array(d[1]), d[2], d[3]) for d in demos[lv]] for lv in iu.LEVELS}
    lens = {lv: [len(d[3]) for d in demos[lv]] for lv in iu.LEVELS}
    cases = [("stable", iu.LEVELS[0], pick(lens[iu.LEVELS[0]], 5, 1, True, repeat=True), 1),
             ("tail", iu.LEVELS[1], pick(lens[iu.LEVELS[1]], 5, 4, False), 4),
             ("one", iu.LEVELS[1], pick(lens[iu.LEVELS[1]], 1, 2, False), 2)]
    for name, level, idx, recurrence in cases:
        logs = []
        for dtype in (torch.float32, torch.float64):
            model = iu.ToyILModel(dtype=dtype, reference_indexing=True)
            model.calls = []
            il = learner(model, preproc, recurrence)
            batch = [packed[level][i] for i in idx]
            log = il.run_epoch_recurrence_one_batch(batch, is_training=True)
            logs.append((log, model.weight.detach().numpy().astype(np.float64), model.calls))
        (log, weight, calls), (log64, weight64, _) = logs
        assert log == log64 and np.array_equal(weight, weight64), "case %s is not exact in float32" % name
        order, ln, inds = reference_structures([packed[level][i] for i in idx])
        pre = "%s/" % name
        out[pre + "level"], out[pre + "indices"], out[pre + "recurrence"] = level, np.array(idx), recurrence
        out[pre + "order"], out[pre + "inds"], out[pre + "lengths"] = np.array([idx[i] for i in order]), inds, np.array(ln)
        F = sum(ln)
        mask = np.ones(F, np.float32)
        mask[inds] = 0
        out[pre + "mask"] = mask
        out[pre + "episode_ids"] = np.repeat(np.arange(len(ln)), ln)
        out[pre + "action_true"] = np.concatenate([np.array(packed[level][idx[i]][3], np.int64) for i in order])
        out[pre + "num_calls"] = len(calls)
        for c, call in enumerate(calls):
            for k, v in call.items():
                out["%scall%d/%s" % (pre, c, k)] = v
        out[pre + "log"] = np.array([log["entropy"], log["policy_loss"], log["accuracy"]], np.float64)
        out[pre + "weight_after"] = weight.astype(np.float32)
        print(name, level, idx, "frames", F, "calls", len(calls), log)
    # a validation epoch: two batches of four demos, every batch a power of two of frames
    level = iu.LEVELS[1]
    groups = [c for c in itertools.combinations(range(N_DEMOS), 4) if pow2(sum(lens[level][i] for i in c))]
    first, second = next((list(a), list(b)) for a in groups for b in groups if not set(a) & set(b) and sum(lens[level][i] for i in a) != sum(lens[level][i] for i in b))
    rest = [i for i in range(N_DEMOS) if i not in first + second]
    model = iu.ToyILModel(reference_indexing=True)
    il = learner(model, preproc, 1, batch_size=4)
    log = il.run_epoch_recurrence(packed[level], is_training=False, indices=first + second + [rest[0]])      # (a trailing partial batch is dropped)
    model64 = iu.ToyILModel(dtype=torch.float64, reference_indexing=True)
    assert learner(model64, preproc, 1, batch_size=4).run_epoch_recurrence(packed[level], is_training=False, indices=first + second + [rest[0]]) == log
    out["epoch/level"], out["epoch/indices"] = level, np.array(first + second + [rest[0]])
    for k in ("entropy", "policy_loss", "accuracy"):
        out["epoch/" + k] = np.array(log[k], np.float64)
    out["epoch/total_frames"] = log["total_frames"]
    print("epoch", log)
    np.savez_compressed(os.path.join(iu.GOLDEN, "cases.npz"), **out)
    with open(os.path.join(iu.GOLDEN, "vocab.json"), "w") as f:
        json.dump(preproc.vocab.vocab, f, sort_keys=True)
        f.write("\n")
    print("wrote", iu.GOLDEN)


if __name__ == "__main__":
    main()
