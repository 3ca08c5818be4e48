"""The level generator against digests RECORDED FROM THE REFERENCE at scale (tests/golden/refpin/gen_digest/, tools/gen_golden_refpin.py gen):
every registered kind, seeds 52000 .. 52511, six consecutive levels each -- 3 072 levels per kind, where the other links of the parity chain
hold a dozen.  A digest covers the grid, the first observation, the agent's pose, max_steps and the mission (refpin_util.level_digest).

  - the engine's host build (bbai_gen.hpp through HostBatch): the whole fixture, levels 0-2 by reset(), 3-5 by the auto-reset of a step;
  - the lane generator's host form (bbai_genl.hpp through hs_generate_lane): the whole fixture of the kinds it covers;
  - the oracle (oracle/levels.py): the first 32 seeds by default, all 512 with BBAI_GEN_DIGEST_FULL=1.

No build of this project stands between the fixture and what is tested; tests/test_gpu_gen_digest.py does the same on the device."""
import ctypes
import os

import numpy as np
import pytest

import refpin_util as rp
from babyai_amd.levels import LEVELS, make_cfg
from hostsim_util import HostBatch, lib
from test_gpu_lane_generator import covered

N, K, SEED0 = rp.GEN_DIGEST_SEEDS, rp.GEN_DIGEST_LEVELS, rp.GEN_DIGEST_SEED0
ORACLE_SEEDS = N if os.environ.get("BBAI_GEN_DIGEST_FULL") == "1" else 32


@pytest.mark.parametrize("name", sorted(LEVELS))
def test_host_build_reproduces_the_reference_digests(name):
    cfg = make_cfg(name)
    hb = HostBatch(cfg, SEED0 + np.arange(N))
    got = np.zeros((N, K), np.uint32)
    for k in range(K):
        if k < 3:
            hb.reset()
        else:
            hb.step(np.full(N, 7, np.uint8))            # 7 = "reset this env now": the auto-reset path
            assert hb.done.all()
        got[:, k] = rp.record_level_digests(cfg, hb.rec, hb.hot, hb.image)
    rp.digest_mismatch(name, got, rp.gen_digest_fixture(name), "host build")


@pytest.mark.parametrize("name", covered())
def test_lane_generator_host_form_reproduces_the_reference_digests(name):
    L = lib()
    cfg = make_cfg(name)
    rec = np.zeros((K, N, cfg.rec_bytes), np.uint8)
    hot = np.zeros((K, N, 16), np.uint8)
    image = np.zeros((K, N, 7, 7, 3), np.uint8)
    mt = np.zeros(624, np.uint32)
    r, h = np.zeros(cfg.rec_bytes, np.uint8), np.zeros(16, np.uint8)
    for i in range(N):
        L.hs_seed(SEED0 + i, mt.ctypes.data)
        mti = ctypes.c_int32(624)
        stale = ctypes.c_uint64(0)
        h[:] = 0
        h[14] = 0xFF                                    # last_locked = none
        for k in range(K):
            rc = L.hs_generate_lane(ctypes.byref(cfg), mt.ctypes.data, ctypes.byref(mti), r.ctypes.data, h.ctypes.data)
            assert rc >= 0, (name, SEED0 + i, k, rc)
            L.hs_observe(ctypes.byref(cfg), r.ctypes.data, h.ctypes.data, image[k, i].ctypes.data)
            L.hs_start_carry(ctypes.byref(cfg), r.ctypes.data, h.ctypes.data, ctypes.byref(stale))
            rec[k, i], hot[k, i] = r, h
    got = np.stack([rp.record_level_digests(cfg, rec[k], hot[k], image[k]) for k in range(K)], axis=1)
    rp.digest_mismatch(name, got, rp.gen_digest_fixture(name), "lane generator, host form")


@pytest.mark.parametrize("name", sorted(LEVELS))
def test_oracle_reproduces_the_reference_digests(name):
    from oracle import levels as olevels
    got = np.zeros((ORACLE_SEEDS, K), np.uint32)
    for i in range(ORACLE_SEEDS):
        env = olevels.make_env(name)
        env.seed(SEED0 + i)
        for k in range(K):
            obs = env.reset()
            got[i, k] = rp.env_level_digest(env, obs)
    rp.digest_mismatch(name, got, rp.gen_digest_fixture(name)[:ORACLE_SEEDS], "oracle")


def test_digest_sees_every_field():
    rng = np.random.RandomState(5)
    grid = rng.randint(0, 256, size=(8, 8)).astype(np.uint8)
    image = rng.randint(0, 256, size=(7, 7, 3)).astype(np.uint8)
    base = dict(grid=grid, image=image, agent=(3, 4, 1), max_steps=64, mission="go to the red ball")
    d0 = rp.level_digest(**base)
    assert d0 == rp.level_digest(**base) and 0 <= d0 < 2 ** 32
    seen = {d0}

    def changed(**kw):
        d = rp.level_digest(**dict(base, **kw))
        assert d not in seen, kw                        # (32-bit values: a chance collision among these few is 1 in 10^8)
        seen.add(d)

    for y, x in ((0, 0), (7, 7), (3, 5)):               # one cell: its type, its colour, its state
        for bit in (1, 8, 64):
            g = grid.copy()
            g[y, x] ^= bit
            changed(grid=g)
    for at in ((0, 0, 0), (6, 6, 2), (3, 6, 1)):        # one observation byte
        im = image.copy()
        im[at] ^= 1
        changed(image=im)
    changed(agent=(4, 4, 1))
    changed(agent=(3, 5, 1))
    changed(agent=(3, 4, 2))                            # the direction
    changed(max_steps=65)
    changed(max_steps=64 + 256)                         # ... and its high byte
    changed(mission="go to the red bell")               # one letter
    changed(mission="go to the red ball ")
    gt = np.ascontiguousarray(grid.T)
    assert not np.array_equal(gt, grid)
    changed(grid=gt)                                    # the same cells in the other order


def test_fixture_is_complete():
    d = rp.golden_path("gen_digest")
    assert sorted(f[:-4] for f in os.listdir(d) if f.endswith(".npy")) == sorted(LEVELS)
    assert len(LEVELS) == 105
    for name in sorted(LEVELS):
        a = rp.gen_digest_fixture(name)
        assert a.shape == (N, K) == (512, 6) and a.dtype == np.uint32, (name, a.shape, a.dtype)
