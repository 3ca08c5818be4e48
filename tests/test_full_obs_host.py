"""The fully observable encoding on the host: the per-cell rule of babyai_amd/csrc/bbai_grid.hpp (full_cell / full_frame, compiled
here for the CPU) on records and poses of the host build of the engine's core, frame for frame against the oracle's
FullyObsWrapper(env).observation(obs)['image'] -- every level, along random-action trajectories across resets; and the new entry
points of the C ABI and the Python argument checks, which need no GPU."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from babyai_amd.levels import LEVELS, make_cfg
from oracle import levels as olevels
from hostsim_util import HostEnv
from test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bbai_observe_full", "bbai_step_full")

_SRC = r"""
#include "bbai_grid.hpp"
using namespace bbai;
extern "C" void fo_frame(const LevelCfg* c, const uint8_t* rec, const Hot* h, uint8_t* out) { full_frame(*c, rec, *h, out); }
"""

NON_SQUARE = sorted(n for n in LEVELS if make_cfg(n).W != make_cfg(n).H)


@pytest.fixture(scope="module")
def full_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("full_rule")
    src, so = str(d / "full_rule.cpp"), str(d / "libfull_rule.so")
    with open(src, "w") as f:
        f.write(_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                           "-I" + os.path.join(ROOT, "babyai_amd", "csrc"), "-o", so, src])
    L = ctypes.CDLL(so)
    P = ctypes.c_void_p
    L.fo_frame.argtypes = [P, P, P, P]
    L.fo_frame.restype = None
    return L


def frame(L, sim):
    c = sim.cfg
    out = np.zeros((c.W, c.H, 3), np.uint8)
    L.fo_frame(ctypes.byref(c), sim.rec.ctypes.data, sim.hot.ctypes.data, out.ctypes.data)
    return out


def wrapped(name):
    from gym_minigrid.wrappers import FullyObsWrapper          # (the oracle's shim: oracle.levels puts it on the path)
    return FullyObsWrapper(olevels.make_env(name))


def drive(L, name, seed, steps):
    """Same seed, same random actions on the wrapped oracle and on the host build; every step's frame compared."""
    ref = wrapped(name)
    ref.seed(seed)
    sim = HostEnv(make_cfg(name), seed)
    rng = random.Random(seed * 7 + 1)
    obs = ref.reset()
    sim.reset()
    resets = 0
    for t in range(steps + 1):
        want = obs["image"]
        assert set(obs) == {"image", "mission"}
        got = frame(L, sim)
        assert got.shape == want.shape == (ref.unwrapped.width, ref.unwrapped.height, 3), (name, seed, t)
        assert np.array_equal(got, want), (name, seed, t, np.argwhere(got != want)[:4].tolist())
        a = rng.randint(0, 6)
        obs, _, d, _ = ref.step(a)
        _, _, done = sim.step(a)
        assert done == bool(d)
        if d:
            obs = ref.reset()
            sim.reset()
            resets += 1
    return resets


@pytest.mark.parametrize("name", sorted(LEVELS))
def test_rule_matches_fully_obs_wrapper(full_lib, name):
    for seed in (5, 1234):
        drive(full_lib, name, seed, 24)


@pytest.mark.parametrize("name", NON_SQUARE)
def test_non_square_levels_longer(full_lib, name):
    resets = 0
    for seed in (11, 12):
        resets += drive(full_lib, name, seed, 150)
    assert make_cfg(name).W != make_cfg(name).H


def test_non_square_levels_are_there():
    assert len(NON_SQUARE) == 19
    assert {"OpenRedDoor", "UnlockToUnlock"} <= set(NON_SQUARE)
    assert (make_cfg("OpenRedDoor").W, make_cfg("OpenRedDoor").H) == (9, 5)
    assert (make_cfg("UnlockToUnlock").W, make_cfg("UnlockToUnlock").H) == (16, 6)


def test_start_carrying_level_at_reset(full_lib):
    """PutNextS5N2Carrying: the reference's reset() puts obj_a into the agent's hands after the 7x7 observation was made and before
    any wrapper observes (bonus_levels.py:821-829), so the full observation of the reset shows obj_a's cell empty while the 7x7 view of
    the same reset may still show the object there."""
    name = "PutNextS5N2Carrying"
    seen_in_view = 0
    for seed in range(40):
        ref = wrapped(name)
        ref.seed(seed)
        plain = olevels.make_env(name)
        plain.seed(seed)
        sim = HostEnv(make_cfg(name), seed)
        obs = ref.reset()
        view = plain.reset()["image"]
        first_view = sim.reset()
        held = ref.unwrapped.carrying
        assert held is not None and held is ref.unwrapped.held_at_start
        got = frame(full_lib, sim)
        assert np.array_equal(got, obs["image"]), seed
        x, y = held.init_pos
        assert tuple(got[x, y]) == (1, 0, 0), seed                     # obj_a's cell: empty in the full observation
        assert np.array_equal(first_view, view), seed                   # the 7x7 view of the same reset, as the reference's
        tc = tuple(held.encode()[:2])
        seen_in_view += any(tuple(v[:2]) == tc for v in view.reshape(-1, 3))
    assert seen_in_view > 0
    drive(full_lib, name, 3, 200)


def test_header_declares_and_library_exports_the_full_obs_entries():
    from babyai_amd import engine
    for name in NAMES:
        assert name in declared_symbols(), name
        assert name in engine.EXPORTED_SYMBOLS, name
    import __graft_entry__
    __graft_entry__.build()
    import torch  # noqa: F401  (torch's HIP runtime first, as the product loads it)
    lib = engine.bind(ctypes.CDLL(os.path.join(ROOT, "babyai_amd", "libbbai_hip.so")))
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.bbai_observe_full(None, None, 1, None, None) == -1                       # BBAI_ERR_ARG: null handle
    assert lib.bbai_step_full(None, None, None, None, None, None, None, 1, None, None) == -1


def test_unknown_pixel_tile_size_raises_without_a_gpu():
    from babyai_amd import vec_env, integrate
    from babyai_amd.engine import BatchedBabyAIEnv
    for make in (lambda **k: BatchedBabyAIEnv("BabyAI-GoToLocal-v0", 4, **k),
                 lambda **k: vec_env.make("BabyAI-GoToLocal-v0", 4, **k),
                 lambda **k: vec_env.BatchedParallelEnv("BabyAI-GoToLocal-v0", 4, **k),
                 lambda **k: vec_env.BatchedManyEnvs("BabyAI-GoToLocal-v0", 4, **k),
                 lambda **k: vec_env.SingleEnv("BabyAI-GoToLocal-v0", **k),
                 lambda **k: integrate.make_envs("BabyAI-GoToLocal-v0", 4, 1, **k)):
        for ts in (12, 0, 64, "8"):
            with pytest.raises(ValueError):
                make(full_obs=True, pixel=True, tile_size=ts)


@pytest.mark.parametrize("name", ["OpenRedDoor", "UnlockToUnlock", "GoToLocal", "BossLevel"])
def test_observation_space_is_the_returned_shape(name):
    """observation_space['image'] of the adapters = the shape of FullyObsWrapper's image / of render('rgb_array', tile_size) (on a
    CPU stand-in engine)."""
    from babyai_amd import vec_env

    class Stub(object):
        pass
    ref = olevels.make_env(name)
    ref.seed(1)
    ref.reset()
    for pixel, ts in ((False, 8), (True, 8), (True, 16), (True, 32)):
        v = vec_env.BatchedParallelEnv("BabyAI-%s-v0" % name, 2, pixel=pixel, engine=Stub(), full_obs=True, tile_size=ts)
        want = wrapped(name).observation_space["image"].shape if not pixel else \
            ref.render("rgb_array", highlight=False, tile_size=ts).shape
        assert v.observation_space["image"].shape == want, (name, pixel, ts)
        assert v[0].observation_space["image"].shape == want
