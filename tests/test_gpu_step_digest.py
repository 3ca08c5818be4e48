"""The DEVICE's step kernels and expert against digests recorded from the reference (tests/golden/refpin/step_digest/, tools/gen_golden_refpin.py
step): every registered kind, 256 envs (seeds 53000 .. 53255, four 64-env blocks), the recorded actions of the reference's own expert with 8 %
random actions -- 128 steps in one room, 320 in several, auto-reset -- and per env and 16-step block a digest over every observation, direction,
float64 reward and done (refpin_util.step_block_digests).  Neither the host build nor the oracle stands in between.

  - test_per_step_and_rollout  k_step: reset(), then T step() calls; before each, bbai_bot_act (k_bot*) must suggest the recorded action wherever
                               the recording says it was the reference expert's own, and 255 where the reference's expert raised.  Then the same
                               actions through bbai_rollout with the stepping lanes' tap on all 256 envs (k_step_ticks), cut as
                               test_gpu_step_every_level.CUTS cuts its calls.
  - test_every_layout          the per-step pass on the eight kinds of SUBSET under every entry of VARIANTS (state layout, consume mode, auto-reset).
                               A batch without auto-reset freezes an env at its first done, where the recording goes on with the next level: there
                               every block before the one that holds the env's first done is compared.

tests/test_step_digest_host.py holds the host build, its expert and the oracle to the same fixture."""
import numpy as np
import pytest

import refpin_util as rp
from babyai_amd.levels import LEVELS
from test_gpu_step_every_level import CUTS, SUBSET, VARIANTS, _make

S, SEED0, B = rp.STEP_DIGEST_STREAMS, rp.STEP_DIGEST_SEED0, rp.STEP_DIGEST_BLOCK


def _per_step(gpu, env, fx, expert):
    """reset() and T step() calls with the recorded actions; outputs collected on the device, copied once.
    -> first digests, block digests, done uint8[T, S], the expert's suggestions uint8[T, S] (or None)."""
    import torch
    acts = torch.as_tensor(fx["actions"], device=gpu)
    steps = acts.shape[0]
    image = torch.zeros((steps, S, 7, 7, 3), dtype=torch.uint8, device=gpu)
    direction = torch.zeros((steps, S), dtype=torch.uint8, device=gpu)
    reward = torch.zeros((steps, S), dtype=torch.float64, device=gpu)
    done = torch.zeros((steps, S), dtype=torch.uint8, device=gpu)
    sug = torch.zeros((steps, S), dtype=torch.uint8, device=gpu) if expert else None
    env.reset()
    first = rp.step_first_digests(env.image.cpu().numpy(), env.direction.cpu().numpy())
    for t in range(steps):
        if expert:
            env.bot_actions(acts[t - 1] if t else None, out=sug[t])
        env.step(acts[t])
        image[t].copy_(env.image)
        direction[t].copy_(env.direction)
        reward[t].copy_(env.reward64)
        done[t].copy_(env.done)
    image, direction, reward, done = (a.cpu().numpy() for a in (image, direction, reward, done))
    return first, rp.step_block_digests(image, direction, reward, done), done, sug.cpu().numpy() if expert else None


def _rollout(gpu, env, fx):
    import torch
    acts = torch.as_tensor(fx["actions"], device=gpu)
    steps = acts.shape[0]
    env.reset()
    first = rp.step_first_digests(env.image.cpu().numpy(), env.direction.cpu().numpy())
    env.set_step_tap(list(range(S)))
    tap = {"image": torch.zeros((steps, S, 7, 7, 3), dtype=torch.uint8, device=gpu), "direction": torch.zeros((steps, S), dtype=torch.uint8, device=gpu),
           "reward64": torch.zeros((steps, S), dtype=torch.float64, device=gpu), "done": torch.zeros((steps, S), dtype=torch.uint8, device=gpu)}
    cuts = [c for c in CUTS if c < steps] + [steps]
    for t0, t1 in zip(cuts, cuts[1:]):
        env.rollout(acts[t0:t1], tap=tap, obs_row0=t0, row0=t0, step_tap=True)
    got = {k: v.cpu().numpy() for k, v in tap.items()}
    return first, rp.step_block_digests(got["image"], got["direction"], got["reward64"], got["done"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LEVELS))
def test_per_step_and_rollout(gpu, name, monkeypatch):
    fx = rp.step_digest_fixture(name)
    seeds = [SEED0 + i for i in range(S)]
    # (read at the expert's first call: room for any subgoal stack T steps can build -- the reference's list is unbounded, the default 48 entries
    # give up on an expert in an unproductive loop, tests/test_hostsim_bot.py test_stack_capacity_is_the_one_documented_divergence)
    monkeypatch.setenv("BBAI_BOT_STACK", "1024")
    env = _make(gpu, name, S, seeds, monkeypatch)
    try:
        first, got, done, sug = _per_step(gpu, env, fx, expert=True)
        assert env.generator_failures() == 0
    finally:
        env.close()
    rp.step_digest_mismatch(name, first, got, fx, "device, per-step calls")
    own, _ = rp.step_digest_expert(name, "device expert", sug, done, fx)
    assert own == int((fx["suggested"] & ~fx["bot_dead"]).sum()) and own > 0, (name, own)
    env = _make(gpu, name, S, seeds, monkeypatch)
    try:
        first, got = _rollout(gpu, env, fx)
        assert env.generator_failures() == 0
    finally:
        env.close()
    rp.step_digest_mismatch(name, first, got, fx, "device, rollout with the stepping lanes' tap")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", SUBSET)
def test_every_layout(gpu, name, variant, monkeypatch):
    fx = rp.step_digest_fixture(name)
    env_vars, opts, auto = VARIANTS[variant]
    env = _make(gpu, name, S, [SEED0 + i for i in range(S)], monkeypatch, env_vars, opts, auto)
    try:
        for k, v in env_vars.items():                  # the intended variant is the one that runs
            if k == "BBAI_INPLACE":
                assert env.get_option("inplace") == int(v), (name, variant)
            if k == "BBAI_CPLANE":
                assert env.get_option("cplane") == 0, (name, variant)
        first, got, done, _ = _per_step(gpu, env, fx, expert=False)
        assert env.generator_failures() == 0
    finally:
        env.close()
    what = "device, per-step calls, " + variant
    if auto:
        rp.step_digest_mismatch(name, first, got, fx, what)
        return
    # frozen at the first done: the blocks before the one that holds it are the recording's, the others are put aside
    ended = done.any(axis=0)
    first_done = np.where(ended, done.argmax(axis=0), done.shape[0])
    live = np.arange(got.shape[1])[None, :] < (first_done // B)[:, None]
    print("%s %s: %d envs froze, %d of %d blocks lie before a first done" % (name, variant, int(ended.sum()), int(live.sum()), live.size))
    assert live.any() and ended.any(), (name, variant)
    rp.step_digest_mismatch(name, first, np.where(live, got, fx["digest"]), fx, what + " (blocks before each env's first done)")
