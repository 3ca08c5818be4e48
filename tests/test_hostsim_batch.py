"""HostBatch (tests/hostsim/hostsim.cpp hs_step_batch: every env of a batch per call, in k_step's order of operations) against N independent
HostEnv loops (one ctypes call per env per step, the reference's order of operations): outputs, records, hot state, stale sets and the
done-action mode's lastStepMatch bits, byte for byte, every step.  HostBatch is the reference tests/test_gpu_step_every_level.py holds the
device's step kernels to, so it has to be exactly the per-env host build first."""
import ctypes

import numpy as np
import pytest

from babyai_amd.levels import make_cfg
from hostsim_util import HostBatch, HostEnv

# a single room, a maze, PutNext with the start carry, BossLevel, a sequenced LevelGen kind, a bonus level
LEVELS = ["GoToLocal", "GoToObjMaze", "PutNextS5N2Carrying", "BossLevel", "SynthSeq", "KeyInBox"]
MODES = [(True, None), (False, None), (True, "done"), (False, "done"), (True, "enum"), (False, "enum")]


class _RefEnv(object):
    """One HostEnv driven as the engine drives an env: action 7 ends the episode, auto-reset or freeze, done-action bits."""

    def __init__(self, cfg, seed, auto_reset, mode):
        self.e = HostEnv(cfg, seed)
        self.auto_reset, self.mode = auto_reset, mode
        self.lsm = ctypes.c_uint32(0)
        self.frozen = False
        self.reward64, self.done = 0.0, 0       # (a reset() leaves the last step's reward and done as they are, as the engine's does)

    def reset(self):
        self.frozen = False
        self.lsm.value = 0
        self.image = self.e.reset()
        self.direction = int(self.e.hot[2])

    def step(self, a):
        if self.frozen:
            return
        e, L = self.e, self.e.L
        rew = ctypes.c_double(0)
        args = (ctypes.byref(e.cfg), e.rec.ctypes.data, e.hot.ctypes.data, ctypes.byref(e.stale), int(a), ctypes.byref(rew))
        if self.mode is None:
            d = L.hs_step64(*args)
        elif self.mode == "done":
            d = L.hs_step64_done(*args, ctypes.byref(self.lsm))
        else:
            d = L.hs_step64_done_enum(*args, ctypes.byref(self.lsm), 0)
        self.reward64, self.done = rew.value, int(d)
        if d and self.auto_reset:
            self.lsm.value = 0
            self.image = e.reset()
        else:
            self.image = e.observe()
            self.frozen = bool(d)
        self.direction = int(e.hot[2])


def _check(level, t, b, refs):
    for i, r in enumerate(refs):
        where = (level, t, i)
        assert np.array_equal(b.image[i], r.image), where
        assert b.direction[i] == r.direction, where
        assert b.reward64[i:i + 1].view(np.uint64)[0] == np.float64(r.reward64).view(np.uint64), where
        assert b.done[i] == r.done, where
        assert np.array_equal(b.rec[i], r.e.rec), where
        h = r.e.hot.copy()
        h[13] = 1 if r.frozen else 0            # (HostEnv keeps no frozen flag; the engine's hot byte 13)
        assert np.array_equal(b.hot[i], h), (where, b.hot[i], h)
        assert int(b.stale[i]) == r.e.stale.value, where
        if b.lsm is not None:
            assert int(b.lsm[i]) == r.lsm.value, where


@pytest.mark.parametrize("auto_reset,mode", MODES, ids=["%s-%s" % ("auto" if a else "frozen", m or "normal") for a, m in MODES])
@pytest.mark.parametrize("level", LEVELS)
def test_host_batch_equals_independent_host_envs(level, auto_reset, mode):
    n, T = 24, 160
    cfg = make_cfg(level)
    seeds = [900 + 7 * i for i in range(n)]
    b = HostBatch(cfg, seeds, auto_reset=auto_reset, done_actions=mode is not None, enum_done=mode == "enum")
    refs = [_RefEnv(cfg, s, auto_reset, mode) for s in seeds]
    rng = np.random.RandomState(len(level) * 31 + MODES.index((auto_reset, mode)))
    ends = {"reward": 0, "reset_cmd": 0, "other": 0}
    for t in range(T):
        if t in (0, 90):                        # (90: a reset() of every env in mid-run, frozen or not)
            b.reset()
            for r in refs:
                r.reset()
            _check(level, t, b, refs)
        # moves and turns mostly, the object actions and done often enough to end episodes both ways; 7 = reset this env
        a = rng.choice(8, size=n, p=[0.15, 0.15, 0.3, 0.12, 0.1, 0.1, 0.05, 0.03]).astype(np.uint8)
        b.step(a)
        for i, r in enumerate(refs):
            was_frozen = r.frozen
            r.step(a[i])
            if not was_frozen and r.done:
                ends["reward" if r.reward64 > 0 else "reset_cmd" if a[i] == 7 else "other"] += 1
        _check(level, t, b, refs)
    assert ends["reset_cmd"] > 0, ends
    if not auto_reset:
        assert b.hot[:, 13].any(), "no env froze"
