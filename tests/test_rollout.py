"""babyai_amd.rollout.DeviceRollout vs the reference's own BaseAlgo.collect_experiences (babyai/rl/algos/base.py:131-260), run
UNMODIFIED on the shim over reference envs in ParallelEnv workers: the experiences the reference collected are recorded by
tools/gen_golden_refpin.py (tests/golden/refpin/rollout.npz) and the device rollout must reproduce them over oracle envs."""
import numpy as np
import pytest
import torch

from rollout_util import OracleTensorEnv, ToyACModel
import refpin_util as rp

FIELDS = rp.ROLLOUT_FIELDS


@pytest.fixture(scope="module")
def rollout_record():
    with np.load(rp.golden_path("rollout.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("level,scale", rp.ROLLOUT_CASES)
def test_device_rollout_equals_reference_collect_experiences(rollout_record, level, scale):
    from babyai_amd.rollout import DeviceRollout
    roll = DeviceRollout(OracleTensorEnv(level, rp.ROLLOUT_SEEDS), ToyACModel(), rp.ROLLOUT_T, 0.99, 0.95, reward_scale=scale)
    total_done = 0
    for it in range(rp.ROLLOUT_ITERS):                     # state carries across rollouts (memory, masks, log tails)
        exps, log = roll.collect_experiences()

        def ref(k):
            return rollout_record[rp.rollout_key(level, scale, it, k)]
        # rewards are shaped from the float64 reward, like the reference: exact for any scale
        for f in FIELDS:
            a, b = torch.from_numpy(ref(f)), getattr(exps, f)
            assert a.shape == b.shape and a.dtype == b.dtype, f
            assert torch.equal(a, b), (level, it, f)
        assert torch.equal(torch.from_numpy(ref("obs.image")), exps.obs.image)
        assert torch.equal(torch.from_numpy(ref("obs.instr")), exps.obs.instr)
        assert int(ref("num_frames")) == log["num_frames"] and int(ref("episodes_done")) == log["episodes_done"]
        assert list(ref("num_frames_per_episode")) == list(log["num_frames_per_episode"])
        for k in ("return_per_episode", "reshaped_return_per_episode"):
            assert np.array_equal(ref(k), np.asarray(log[k], dtype=np.float64)), k
        total_done += log["episodes_done"]
    assert total_done >= 5                                 # the comparison crossed auto-resets


def test_collect_experiences_copy_survives_the_next_collection():
    """`exps` of collect_experiences() alias the collector's buffers (module docstring); copy=True hands out tensors of
    the caller's own, like the reference's fresh transposed copies (base.py:207-232)."""
    from babyai_amd.rollout import DeviceRollout
    seeds = [900 + i for i in range(4)]
    roll = DeviceRollout(OracleTensorEnv("GoToObjS4", seeds), ToyACModel(), 12, 0.99, 0.95, reward_scale=20.0)
    views, _ = roll.collect_experiences()
    own, _ = roll_b = DeviceRollout(OracleTensorEnv("GoToObjS4", seeds), ToyACModel(), 12, 0.99, 0.95, reward_scale=20.0).collect_experiences(copy=True)
    for f in FIELDS:
        assert torch.equal(getattr(views, f), getattr(own, f)), f
    keep = {f: getattr(own, f).clone() for f in FIELDS}
    keep_img = own.obs.image.clone()
    assert views.value.data_ptr() == roll.values.data_ptr() and own.value.data_ptr() != roll.values.data_ptr()
    before = views.action.clone()
    roll.collect_experiences()                             # overwrites what `views` points at ...
    assert not torch.equal(views.action, before) or not torch.equal(views.value, keep["value"])
    for f in FIELDS:                                       # ... and leaves the copies alone
        assert torch.equal(getattr(own, f), keep[f]), f
    assert torch.equal(own.obs.image, keep_img)
