"""The egocentric observation at view sizes 3, 5, 7, 9, 11 on the host: the per-cell rule of babyai_amd/csrc/bbai_viewn.hpp (observe_env_n, and
observe_env_staged_n -- the loads and lookups k_view_obs<V> makes -- compiled here for the CPU) on records and poses of the host build of the
engine's core, frame for frame against the oracle env with agent_view_size = V set before seed() / reset() (what ViewSizeWrapper(env, V)
does) -- every level, along random-action trajectories across resets; and the new entry points of the C ABI and the Python argument
checks, which need no GPU."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

from babyai_amd.levels import LEVELS, make_cfg
from oracle import levels as olevels
from hostsim_util import HostEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bbai_observe_view", "bbai_step_view")
HEADER = os.path.join(ROOT, "include", "bbai_view_size.h")
SIZES = (3, 5, 7, 9, 11)
OTHER = (3, 5, 9, 11)

_SRC = r"""
#include "bbai_viewn.hpp"
using namespace bbai;
extern "C" void vn_frame(const LevelCfg* c, const uint8_t* rec, const Hot* h, int V, uint8_t* out) { observe_env_n(*c, rec, *h, V, out); }
extern "C" void vn_staged(const LevelCfg* c, const uint8_t* rec, const Hot* h, int V, uint8_t* out) { observe_env_staged_n(*c, rec, *h, V, out); }
extern "C" void vn_vis(int V, const uint32_t* opq, uint32_t* vis) { process_vis_rows_n(V, opq, vis); }
extern "C" void vn_vis7(const uint32_t* opq, uint32_t* vis) { process_vis_rows(opq, vis); }
extern "C" int vn_max_dword(const LevelCfg* c, int V) {
    // the largest record dword the staged window can ask for, over every pose -- also poses no level produces
    int hi = -1, lo = 1 << 30;
    for (int ax = 0; ax < 256; ++ax) for (int ay = 0; ay < 256; ++ay) for (int d = 0; d < 4; ++d) {
        int tx, ty; view_top_left_n(V, ax, ay, d, tx, ty);
        for (int r = 0; r < V; ++r) for (int k = 0; k < view_nd(V); ++k) {
            const int i = view_win_dword(*c, tx, ty, r, k);
            hi = i > hi ? i : hi; lo = i < lo ? i : lo;
        }
    }
    return lo < 0 ? -1 : hi;
}
"""


@pytest.fixture(scope="module")
def view_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("view_rule")
    src, so = str(d / "view_rule.cpp"), str(d / "libview_rule.so")
    with open(src, "w") as f:
        f.write(_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                           "-I" + os.path.join(ROOT, "babyai_amd", "csrc"), "-o", so, src])
    L = ctypes.CDLL(so)
    P = ctypes.c_void_p
    L.vn_frame.argtypes = L.vn_staged.argtypes = [P, P, P, ctypes.c_int, P]
    L.vn_frame.restype = L.vn_staged.restype = None
    L.vn_vis.argtypes = [ctypes.c_int, P, P]
    L.vn_vis7.argtypes = [P, P]
    L.vn_max_dword.argtypes = [P, ctypes.c_int]
    return L


def frame(L, sim, V, staged=False):
    # the record in a buffer of exactly its size (the staged form must not read outside the appearance plane, let alone the record)
    out = np.zeros((V, V, 3), np.uint8)
    (L.vn_staged if staged else L.vn_frame)(ctypes.byref(sim.cfg), sim.rec.ctypes.data, sim.hot.ctypes.data, V, out.ctypes.data)
    return out


def oracle_env(name, seed, V):
    e = olevels.make_env(name)
    e.agent_view_size = V
    e.seed(seed)
    return e


def drive(L, name, seed, steps, sizes=OTHER):
    """Same seed, same random actions on one oracle env per view size and on the host build; every step's frames compared."""
    refs = {V: oracle_env(name, seed, V) for V in sizes}
    sim = HostEnv(make_cfg(name), seed)
    rng = random.Random(seed * 7 + 1)
    obs = {V: r.reset() for V, r in refs.items()}
    img7 = sim.reset()
    resets = 0
    for t in range(steps + 1):
        for V in sizes:
            want = obs[V]["image"]
            got = frame(L, sim, V)
            assert got.shape == want.shape == (V, V, 3), (name, seed, t, V)
            assert np.array_equal(got, want), (name, seed, t, V, np.argwhere(got != want)[:4].tolist())
        for V in SIZES:
            assert np.array_equal(frame(L, sim, V, staged=True), frame(L, sim, V)), (name, seed, t, V)
        assert np.array_equal(frame(L, sim, 7), img7), (name, seed, t)          # V = 7: the bytes the step's own observe_env wrote
        a = rng.randint(0, 6)
        dones = set()
        for V, r in refs.items():
            obs[V], _, d, _ = r.step(a)
            dones.add(bool(d))
        img7, _, done = sim.step(a)
        assert dones == {done}, (name, seed, t)
        if done:
            obs = {V: r.reset() for V, r in refs.items()}
            img7 = sim.reset()
            resets += 1
    return resets


@pytest.mark.parametrize("name", sorted(LEVELS))
def test_rule_matches_the_oracle_at_every_view_size(view_lib, name):
    for seed in (5, 1234):
        drive(view_lib, name, seed, 24)


def test_all_levels_are_covered():
    assert len(LEVELS) == 105


@pytest.mark.parametrize("name", ["GoToObjS4", "GoToLocalS5N2", "OpenRedDoor", "BossLevel"])
def test_longer_runs_cross_resets(view_lib, name):
    resets = drive(view_lib, name, 11, 150)
    if name in ("GoToObjS4", "GoToLocalS5N2"):      # max_steps 16 / 25
        assert resets >= 5


def test_view_size_7_is_observe_env(view_lib):
    """observe_env_n at 7 = bbai_step.hpp observe_env on the same states, and process_vis_rows_n at 7 = process_vis_rows on every pattern
    of a few random row sets."""
    for name in ("GoToLocal", "BossLevel", "OpenRedDoor", "GoToObjS4", "KeyCorridorS3R1"):
        sim = HostEnv(make_cfg(name), 77)
        rng = random.Random(3)
        img = sim.reset()
        for t in range(120):
            assert np.array_equal(frame(view_lib, sim, 7), img), (name, t)
            img, _, done = sim.step(rng.randint(0, 6))
            if done:
                img = sim.reset()
    rs = np.random.RandomState(0)
    for _ in range(2000):
        opq = rs.randint(0, 128, size=7).astype(np.uint32)
        a, b = np.zeros(7, np.uint32), np.zeros(7, np.uint32)
        view_lib.vn_vis(7, opq.ctypes.data, a.ctypes.data)
        view_lib.vn_vis7(opq.ctypes.data, b.ctypes.data)
        assert np.array_equal(a, b), opq


def test_staged_window_stays_inside_the_appearance_plane(view_lib):
    """Every dword the staged form can ask for, whatever the pose bytes hold, lies inside the record's appearance plane."""
    for name in ("GoToObjS4", "GoToLocalS5N2", "GoToLocal", "OpenRedDoor", "UnlockToUnlock", "BossLevel"):
        c = make_cfg(name)
        for V in SIZES:
            hi = view_lib.vn_max_dword(ctypes.byref(c), V)
            assert 0 <= hi < c.ES * c.EH // 4, (name, V, hi)


def test_start_carrying_level_at_reset(view_lib):
    """PutNextS5N2Carrying: the reference's reset() builds its observation before it puts obj_a into the agent's hands
    (bonus_levels.py:821-829) and ViewSizeWrapper does not observe again: the reset frame shows the object on its cell and the agent's cell
    empty; from the first step on the agent's cell shows what it carries."""
    name = "PutNextS5N2Carrying"
    seen = {V: 0 for V in OTHER}
    for seed in range(40):
        for V in OTHER:
            ref = oracle_env(name, seed, V)
            sim = HostEnv(make_cfg(name), seed)
            obs = ref.reset()
            sim.reset()
            held = ref.unwrapped.carrying
            assert held is not None
            got = frame(view_lib, sim, V)
            assert np.array_equal(got, obs["image"]), (seed, V)
            assert np.array_equal(frame(view_lib, sim, V, staged=True), got), (seed, V)
            assert tuple(got[V // 2, V - 1]) == (1, 0, 0), (seed, V)          # the agent's cell: empty, nothing carried yet
            # where the object's cell is inside the view (a 5x5 room: a window of 9 or 11 always holds it unless a wall hides it)
            x, y = held.init_pos
            ax, ay = ref.unwrapped.agent_pos
            fx, fy = ref.unwrapped.dir_vec
            rx, ry = -fy, fx
            dx, dy = x - ax, y - ay
            vj, vi = V - 1 - (dx * fx + dy * fy), V // 2 + (dx * rx + dy * ry)
            if 0 <= vi < V and 0 <= vj < V:
                assert tuple(got[vi, vj]) == tuple(held.encode()), (seed, V)      # (an open room: nothing hides it)
                seen[V] += 1
    assert all(v > 0 for v in seen.values()), seen
    drive(view_lib, name, 3, 100)


def prototypes():
    """{entry: [kind of every parameter]} of include/bbai_view_size.h; kinds "ptr", "i64", "int"."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(bbai_[a-z_]+)\s*\(([^)]*)\)\s*;", text):
        assert ret.strip() == "int" and name not in out, name
        kinds = []
        for p in params.split(","):
            words = [w for w in p.split() if w != "const"]
            kinds.append("ptr" if "*" in p else {"int64_t": "i64", "int": "int"}[words[0]])
        out[name] = kinds
    return out


def test_every_view_prototype_has_its_table_row():
    """The header against engine.ABI_VIEW, prototype by prototype (tests/test_binding_host.py does the same for include/bbai.h and ABI);
    bbai_step_view begins as every stepping entry does."""
    from babyai_amd import engine
    protos = prototypes()
    assert list(protos) == list(NAMES) == list(engine.ABI_VIEW)
    assert engine.VIEW_SYMBOLS == tuple(engine.ABI_VIEW) and not set(engine.ABI_VIEW) & (set(engine.ABI) | set(engine.ABI_REPLAY))
    kind = {ctypes.c_void_p: "ptr", ctypes.c_int64: "i64", ctypes.c_int: "int"}
    for name, params in protos.items():
        restype, argtypes = engine.ABI_VIEW[name]
        assert restype is ctypes.c_int and [kind[t] for t in argtypes] == params, name
    step = engine.ABI["bbai_step"][1]
    assert engine.ABI_VIEW["bbai_step_view"][1][:len(step) - 1] == step[:-1]           # (bbai_step's arguments but its stream)
    subprocess.check_call(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", HEADER])
    text = open(HEADER).read()
    assert "ViewSizeWrapper" in text and "levelgen.py:25-33" in text


def test_header_declares_and_library_exports_the_view_entries():
    from babyai_amd import engine
    for name in NAMES:
        assert name in prototypes(), name
        assert name in engine.VIEW_SYMBOLS, name
    import __graft_entry__
    __graft_entry__.build()
    import torch  # noqa: F401  (torch's HIP runtime first, as the product loads it)
    lib = engine.bind(ctypes.CDLL(os.path.join(ROOT, "babyai_amd", "libbbai_hip.so")))
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.bbai_observe_view(None, 9, None, 1, None, None) == -1                       # BBAI_ERR_ARG: null handle
    assert lib.bbai_step_view(None, None, None, None, None, None, None, 1, 9, None, None) == -1


def _makers():
    from babyai_amd import vec_env, integrate
    from babyai_amd.engine import BatchedBabyAIEnv
    return (lambda **k: BatchedBabyAIEnv("BabyAI-GoToLocal-v0", 4, **k),
            lambda **k: vec_env.make("BabyAI-GoToLocal-v0", 4, **k),
            lambda **k: vec_env.BatchedParallelEnv("BabyAI-GoToLocal-v0", 4, **k),
            lambda **k: vec_env.BatchedManyEnvs("BabyAI-GoToLocal-v0", 4, **k),
            lambda **k: vec_env.SingleEnv("BabyAI-GoToLocal-v0", **k),
            lambda **k: integrate.make_envs("BabyAI-GoToLocal-v0", 4, 1, **k))


def test_bad_view_sizes_raise_without_a_gpu():
    for make in _makers():
        for v in (4, 6, 8, 10, 1, 13, 0, -3, "9", 9.0, None, True):
            with pytest.raises(ValueError):
                make(view_size=v)


def test_view_size_goes_with_neither_pixels_nor_full_obs():
    for make in _makers():
        for v in OTHER:
            with pytest.raises(ValueError):
                make(view_size=v, pixel=True)
            with pytest.raises(ValueError):
                make(view_size=v, full_obs=True)
            with pytest.raises(ValueError):
                make(view_size=v, full_obs=True, pixel=True, tile_size=16)


@pytest.mark.parametrize("name", ["GoToLocal", "BossLevel", "OpenRedDoor", "GoToObjS4"])
def test_observation_space_is_the_oracle_image_shape(name):
    from babyai_amd import vec_env

    class Stub(object):
        pass
    for V in SIZES:
        ref = oracle_env(name, 1, V)
        want = ref.reset()["image"].shape
        assert want == (V, V, 3)
        for cls in (vec_env.BatchedParallelEnv, vec_env.BatchedManyEnvs):
            v = cls("BabyAI-%s-v0" % name, 2, engine=Stub(), view_size=V)
            assert v.observation_space["image"].shape == want, (name, V)
            assert v[0].observation_space["image"].shape == want
    assert vec_env.BatchedParallelEnv("BabyAI-%s-v0" % name, 2, engine=Stub()).observation_space["image"].shape == (7, 7, 3)
