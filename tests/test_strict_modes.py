"""`strict` verifier modes that no registered level switches on (babyai/levels/verifier.py:398-401 PutNextInstr,
:466-469 BeforeInstr, :507-510 AfterInstr): flipped on by hand after every reset in the stand-alone oracle and in the kernel core
(host build of bbai_step.hpp), stepped side by side, and pinned to the REFERENCE's own instruction objects under the same
protocol through the records of tools/gen_golden_refpin.py (tests/golden/refpin/strict_modes.json)."""
import numpy as np
import pytest

from oracle import levels as olevels
from babyai_amd.levels import make_cfg
from hostsim_util import HostEnv
import refpin_util as rp

PROG_STRICT = 103          # byte offset of Prog.strict inside the 112-byte program (bbai_types.hpp)


@pytest.fixture(scope="module")
def strict_record():
    return rp.load_json("strict_modes.json")


@pytest.mark.parametrize("name,leaf_bits,seq", rp.STRICT_CASES)
def test_strict_modes_three_way(strict_record, name, leaf_bits, seq):
    cur = {}

    class HostTwin(object):
        """The kernel core next to the oracle: the same observations, float32 rewards and dones at every step."""

        def __init__(self, seed):
            self.host = HostEnv(make_cfg(name), seed)
            self.seed = seed
            cur["host"] = self.host

        def reset(self, obs):
            assert np.array_equal(obs["image"], self.host.reset()), (name, self.seed)

        def step(self, act, obs, reward, done):
            img, rh, dh = self.host.step(act)
            assert np.array_equal(obs["image"], img), (name, self.seed)
            assert np.float32(reward) == rh and done == dh, (name, self.seed)

    def env_for_seed(seed):
        ora = olevels.make_env(name)
        ora.seed(seed)
        return ora

    def arm(ora):
        """Switch strict on in both after a reset (the reference: a SeqInstr that is not an AndInstr / every leaf)."""
        host = cur["host"]
        if seq and isinstance(ora.instrs, olevels.Combo) and ora.instrs.how != "and":
            ora.instrs.strict = True
            host.rec[host.cfg.off_prog + PROG_STRICT] |= 16
        if leaf_bits:
            for leaf in olevels._leaves(ora.instrs):
                leaf.strict = True
            host.rec[host.cfg.off_prog + PROG_STRICT] |= 15

    got, want = rp.strict_episodes(env_for_seed, arm, twin=HostTwin), strict_record[name]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (name, w["seed"], w["ep"])
    assert any(r["strict_failure"] for r in got), "the strict branches were never taken"
