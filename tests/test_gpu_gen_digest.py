"""The DEVICE's level generator against digests recorded from the reference (tests/golden/refpin/gen_digest/, tools/gen_golden_refpin.py gen):
every registered kind, 512 envs (seeds 52000 .. 52511) x six consecutive levels -- three by reset(), three out of the look-ahead ring through the
step path (action 7 for every env: k_pregen into ring slots, then k_consume / the fused consume / the in-place advance).  Neither the host build
nor the oracle stands in between: all 3 072 digests (refpin_util.level_digest: grid, first observation, pose, max_steps, mission) per kind must
equal the reference's.  512 x 6 is not reduced: the generator fault test_gpu_lane_generator.py describes showed in 3 of 1 024 levels.

Three forms: the default generator and layout on every kind; each generator forced (BBAI_PREGEN_LANE) on the kinds the lane generator covers;
each state layout forced (BBAI_INPLACE) on a short list.  tests/test_gen_digest_host.py holds the host build and the oracle to the same fixture."""
import os

import numpy as np
import pytest

import refpin_util as rp
from babyai_amd.levels import LEVELS
from test_gpu_lane_generator import covered

N, K, SEED0 = rp.GEN_DIGEST_SEEDS, rp.GEN_DIGEST_LEVELS, rp.GEN_DIGEST_SEED0
LAYOUT_KINDS = ["GoToLocal", "PickupLoc", "GoTo", "BossLevel", "SynthS5R2", "PutNextS5N2Carrying", "KeyInBox", "UnlockToUnlock"]


def _digests(env, name, gpu, what):
    """Six generator rounds of `env` against the fixture; closes the env."""
    import torch
    try:
        got = np.zeros((N, K), np.uint32)
        reset_all = torch.full((N,), 7, dtype=torch.uint8, device=gpu)      # 7 = "reset this env now"
        for k in range(K):
            if k < 3:
                env.reset()
            else:
                env.step(reset_all)
            rec, hot, _ = env.export_state()
            got[:, k] = rp.record_level_digests(env.cfg, rec, hot, env.image.cpu().numpy(), env.missions())
        rp.digest_mismatch(name, got, rp.gen_digest_fixture(name), what)
        assert env.generator_failures() == 0 and env.gate_timeouts() == 0
    finally:
        env.close()


def _make(name, gpu, var=None, value=None):
    """BatchedBabyAIEnv(name, 512, seeds=52000), created with the environment variable `var` = `value` (and put back)."""
    from babyai_amd.engine import BatchedBabyAIEnv
    old = os.environ.get(var) if var else None
    if var:
        os.environ[var] = value
    try:
        return BatchedBabyAIEnv("BabyAI-%s-v0" % name, N, device=gpu, seeds=SEED0)
    finally:
        if var and old is None:
            del os.environ[var]
        elif var:
            os.environ[var] = old


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LEVELS))
def test_device_generator_reproduces_the_reference_digests(gpu, name):
    _digests(_make(name, gpu), name, gpu, "device")


@pytest.mark.gpu
@pytest.mark.parametrize("lane", [0, 1])
@pytest.mark.parametrize("name", covered())
def test_each_generator_reproduces_the_reference_digests(gpu, name, lane):
    env = _make(name, gpu, "BBAI_PREGEN_LANE", str(lane))
    if env.get_option("pregen_lane") != lane:
        uncovered = lane == 1 and env.get_option("inplace") == 1 and env.get_option("cplane") == 0
        env.close()
        if uncovered:       # (as test_gpu_lane_generator._run: BBAI_INPLACE=1 forced on a kind whose default is the classic layout)
            pytest.skip("%s in the in-place layout without a C plane: not covered by the lane generator (bbai_create)" % name)
        raise AssertionError("%s: BBAI_PREGEN_LANE=%d did not select that generator" % (name, lane))
    _digests(env, name, gpu, "device, BBAI_PREGEN_LANE=%d" % lane)


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", [0, 1])
@pytest.mark.parametrize("name", LAYOUT_KINDS)
def test_each_state_layout_reproduces_the_reference_digests(gpu, name, inplace, monkeypatch):
    from babyai_amd.engine import BatchedBabyAIEnv
    monkeypatch.setenv("BBAI_INPLACE", str(inplace))
    env = BatchedBabyAIEnv("BabyAI-%s-v0" % name, N, device=gpu, seeds=SEED0)
    if env.get_option("inplace") != inplace:
        env.close()
        raise AssertionError("%s: BBAI_INPLACE=%d did not take effect" % (name, inplace))
    _digests(env, name, gpu, "device, BBAI_INPLACE=%d" % inplace)
