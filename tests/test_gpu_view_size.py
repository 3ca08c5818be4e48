"""Observations at view sizes 3, 5, 9, 11 on the device (view_size=V; k_view_obs<V>, include/bbai_view_size.h bbai_observe_view / bbai_step_view): byte
for byte against oracle envs with agent_view_size = V set before seed() / reset() -- what ViewSizeWrapper(env, V) does -- driven the same
way (same seeds, same actions; auto-reset as the reference's ParallelEnv, frozen envs as ManyEnvs), over both state layouts, held envs,
rollouts, snapshots, reseeds, checkpoints, imports, streams, the list-of-dicts adapter and DeviceRollout; and nothing else moves.
n = 200 envs: not a multiple of 64 or 16, and 200 * 3 V^2 is no multiple of 16 at any of the sizes, so the byte tail of the store runs."""
import ctypes
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 200
STEPS = 40
SIZES = (3, 5, 9, 11)
SEED = 1000
_rs = np.random.RandomState(12)
TRACKED = np.sort(np.concatenate([[0, 63, 64, 127, 128, 199],
                                  _rs.choice(np.setdiff1d(np.arange(N), [0, 63, 64, 127, 128, 199]), 58, replace=False)]))
ACTS = np.random.RandomState(13).randint(0, 7, size=(STEPS, N)).astype(np.uint8)
assert len(TRACKED) == 64 and all(N * 3 * v * v % 16 for v in SIZES + (7,))


def oracle_env(level, seed, V):
    from oracle import levels as olevels
    e = olevels.make_env(level)
    e.agent_view_size = V
    e.seed(int(seed))
    return e


_ORACLE = {}


def oracle_run(level, V, auto_reset, seed=SEED):
    """One oracle env per tracked env, stepped with ACTS: frames [STEPS + 1, 64, V, V, 3] (reset, then after every step), dones and which
    steps each env really took (a frozen env takes none).  Computed once per case and shared."""
    key = (level, V, auto_reset, seed)
    if key not in _ORACLE:
        envs = [oracle_env(level, seed + int(i), V) for i in TRACKED]
        last = [e.reset()["image"] for e in envs]
        frames = [np.stack(last)]
        dones = np.zeros((STEPS, len(envs)), bool)
        live = np.ones((STEPS, len(envs)), bool)
        frozen = np.zeros(len(envs), bool)
        for t in range(STEPS):
            for j, e in enumerate(envs):
                live[t, j] = not frozen[j]
                if frozen[j]:
                    continue
                o, _, d, _ = e.step(int(ACTS[t, TRACKED[j]]))
                if d:
                    dones[t, j] = True
                    if auto_reset:
                        o = e.reset()
                    else:
                        frozen[j] = True
                last[j] = o["image"]
            frames.append(np.stack(last))
        for a in (dones, live):
            a.setflags(write=False)
        fr = np.stack(frames)
        fr.setflags(write=False)
        _ORACLE[key] = (fr, dones, live)
    return _ORACLE[key]


def make(gpu, level, seed=SEED, n=N, **kw):
    from babyai_amd.engine import BatchedBabyAIEnv
    return BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device=gpu, seeds=seed, **kw)


def run_against_oracle(gpu, level, V, auto_reset):
    import torch
    want, wdone, live = oracle_run(level, V, auto_reset)
    env = make(gpu, level, auto_reset=auto_reset, view_size=V)
    sel = torch.as_tensor(TRACKED, device=gpu)
    obs = env.reset()
    assert obs["image"].data_ptr() == env.view.data_ptr() and tuple(env.view.shape) == (N, V, V, 3)
    assert tuple(env.image.shape) == (N, 7, 7, 3)
    got = np.zeros((STEPS + 1, len(TRACKED), V, V, 3), np.uint8)
    dn = np.zeros((STEPS, len(TRACKED)), bool)
    got[0] = obs["image"][sel].cpu().numpy()
    dev_acts = torch.as_tensor(ACTS, device=gpu)
    for t in range(STEPS):
        obs, _, done, _ = env.step(dev_acts[t])
        assert obs["image"].data_ptr() == env.view.data_ptr()
        got[t + 1] = obs["image"][sel].cpu().numpy()
        dn[t] = done[sel].cpu().numpy().astype(bool)
    layout = env.get_option("inplace")
    env.close()
    assert np.array_equal(dn[live], wdone[live]), (level, np.argwhere(dn != wdone)[:4].tolist())
    for t in range(STEPS + 1):
        if not np.array_equal(got[t], want[t]):
            bad = np.argwhere((got[t] != want[t]).any(axis=(1, 2, 3)))[:4, 0]
            raise AssertionError((level, V, auto_reset, t, [int(TRACKED[b]) for b in bad]))
    return layout, wdone


@pytest.mark.gpu
@pytest.mark.parametrize("V", SIZES)
@pytest.mark.parametrize("level,inplace", [("GoToObjS4", None), ("GoToLocalS5N2", "0"), ("GoToLocalS5N2", "1"), ("OpenRedDoor", None),
                                           ("PutNextS5N2Carrying", None), ("BossLevel", None)])
def test_frames_match_the_oracle(gpu, level, inplace, V, monkeypatch):
    if inplace is not None:
        monkeypatch.setenv("BBAI_INPLACE", inplace)
    layout, wdone = run_against_oracle(gpu, level, V, True)
    if inplace is not None:
        assert layout == int(inplace)
    if level in ("GoToObjS4", "GoToLocalS5N2"):
        assert wdone.any(axis=0).all()          # max_steps 16 / 25: every tracked env finished and showed a next episode's first frame


@pytest.mark.gpu
@pytest.mark.parametrize("V", SIZES)
def test_frozen_envs_keep_their_final_frame(gpu, V):
    _, wdone = run_against_oracle(gpu, "GoToObjS4", V, False)
    assert wdone.any(axis=0).all()


@pytest.mark.gpu
def test_view_size_7_is_the_step_image(gpu):
    import torch
    env = make(gpu, "BossLevel", seed=31)
    assert env.view is None
    env.reset()
    rng = np.random.RandomState(2)
    for t in range(60):
        env.step(torch.as_tensor(rng.randint(0, 7, size=N).astype(np.uint8), device=gpu))
        assert torch.equal(env.observe_view(view_size=7), env.image), t
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("level", ["BossLevel", "GoToLocal"])
def test_nothing_else_moves(gpu, level):
    """Same seeds, same actions: the 7x7 image, direction, reward, reward64 and done are byte-identical with and without view_size=9."""
    import torch
    a, b = make(gpu, level, seed=41), make(gpu, level, seed=41, view_size=9)
    oa, ob = a.reset(), b.reset()
    assert torch.equal(a.image, b.image) and torch.equal(oa["direction"], ob["direction"])
    rng = np.random.RandomState(2)
    for t in range(STEPS):
        act = torch.as_tensor(rng.randint(0, 7, size=N).astype(np.uint8), device=gpu)
        oa, _, _, _ = a.step(act)
        ob, _, _, _ = b.step(act)
        assert torch.equal(oa["direction"], ob["direction"]), t
        for x, y in ((a.image, b.image), (a.direction, b.direction), (a.reward, b.reward), (a.reward64, b.reward64), (a.done, b.done)):
            assert torch.equal(x, y), t
    a.close()
    b.close()


@pytest.mark.gpu
def test_held_envs_keep_their_frame(gpu):
    import torch
    V = 9
    env, twin = make(gpu, "GoToLocalS5N2", view_size=V), make(gpu, "GoToLocalS5N2", view_size=V)
    env.reset()
    twin.reset()
    rng = np.random.RandomState(5)
    for t in range(STEPS):
        ids = np.sort(rng.choice(N, 70, replace=False))
        acts = rng.randint(0, 7, size=len(ids)).astype(np.uint8)
        before = env.view.clone()
        obs, _, _, _ = env.step(acts, ids=ids)
        held = np.setdiff1d(np.arange(N), ids)
        assert obs["image"].data_ptr() == env.view.data_ptr()
        assert torch.equal(env.view[held], before[held]), t
        # the listed envs: what a twin shows whose other envs hold through a full action vector
        full = np.full(N, twin.HOLD, np.uint8)
        full[ids] = acts
        twin.set_option("step_hold", 1)
        twin.step(torch.as_tensor(full, device=gpu))
        assert torch.equal(env.view, twin.view), t
    env.close()
    twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("level", ["BossLevel", "GoToLocalS5N2"])
def test_rollout_final_frame_is_t_steps(gpu, level):
    import torch
    T = 24
    a, b = make(gpu, level, seed=9, view_size=11), make(gpu, level, seed=9, view_size=11)
    a.reset()
    b.reset()
    acts = torch.as_tensor(ACTS[:T].copy(), device=gpu)
    oa = a.rollout(acts)
    for t in range(T):
        b.step(acts[t])
    assert oa["image"].data_ptr() == a.view.data_ptr()
    assert torch.equal(a.view, b.view) and torch.equal(a.image, b.image) and torch.equal(a.done, b.done)
    a.close()
    b.close()


@pytest.mark.gpu
def test_state_moves_reproduce_the_oracle_frame(gpu):
    """load_state, reseed, checkpoint + observe_view(), import_state: the frames of oracle envs stepped alongside."""
    import torch
    level, V, n, seed = "OpenRedDoor", 9, 48, 4242
    env = make(gpu, level, seed=seed, n=n, view_size=V)
    refs = [oracle_env(level, seed + i, V) for i in range(n)]
    last = [r.reset()["image"] for r in refs]
    env.reset()
    rng = np.random.RandomState(8)

    def step():
        a = rng.randint(0, 7, size=n).astype(np.uint8)
        _, _, done, _ = env.step(torch.as_tensor(a, device=gpu))
        dn = done.cpu().numpy()
        for i, r in enumerate(refs):
            o, _, d, _ = r.step(int(a[i]))
            assert bool(d) == bool(dn[i])
            last[i] = r.reset()["image"] if d else o["image"]

    for t in range(6):
        step()
    assert np.array_equal(env.view.cpu().numpy(), np.stack(last))
    # load_state: envs 40..47 take the states of envs 0..7; the returned rows of the listed envs are their frames
    snap = env.save_state(np.arange(8))
    obs = env.load_state(snap, ids=np.arange(40, 48))
    assert obs["image"].data_ptr() == env.view.data_ptr()
    got = obs["image"].cpu().numpy()
    assert np.array_equal(got[40:48], np.stack(last[:8])) and np.array_equal(got[:40], np.stack(last[:40]))
    # reseed: envs 40..47 start the first level of new seeds
    new = [oracle_env(level, 900 + k, V) for k in range(8)]
    obs = env.reseed(np.arange(40, 48), [900 + k for k in range(8)])
    for k in range(8):
        refs[40 + k] = new[k]
        last[40 + k] = new[k].reset()["image"]
    assert np.array_equal(obs["image"].cpu().numpy(), np.stack(last))
    for t in range(4):
        step()
    assert np.array_equal(env.view.cpu().numpy(), np.stack(last))
    # checkpoint into another batch: the blob does not carry the observation, observe_view() draws it
    blob = env.save_checkpoint()
    other = make(gpu, level, seed=1, n=n, view_size=V)
    other.reset()
    other.load_checkpoint(blob)
    assert not torch.equal(other.view, env.view)
    assert other.observe_view().data_ptr() == other.view.data_ptr()
    assert torch.equal(other.view, env.view)
    for t in range(3):
        step()
    other.import_state(*env.export_state())
    other.observe_view()
    assert np.array_equal(other.view.cpu().numpy(), np.stack(last))
    for v in (3, 5, 11):            # any size from any batch
        fr = other.observe_view([0, n - 1], view_size=v).cpu().numpy()
        assert fr.shape == (2, v, v, 3)
    other.close()
    env.close()


@pytest.mark.gpu
def test_id_lists_refusals_and_a_side_stream(gpu):
    import torch
    level, V, n = "OpenRedDoor", 9, N
    env = make(gpu, level, seed=5, view_size=V)
    env.reset()
    want = {i: oracle_env(level, 5 + i, V).reset()["image"] for i in (0, 3)}
    fr = env.observe_view([-1, n, 1 << 40, 3, 0, 3]).cpu().numpy()
    assert fr.shape == (6, V, V, 3)
    assert not fr[:3].any()
    assert np.array_equal(fr[3], want[3]) and np.array_equal(fr[4], want[0]) and np.array_equal(fr[5], want[3])
    assert env.observe_view([]).shape == (0, V, V, 3)
    with pytest.raises(ValueError):
        env.observe_view(None, out=torch.zeros((n - 1, V, V, 3), dtype=torch.uint8, device=gpu))
    for bad in (4, 13):
        with pytest.raises(ValueError):
            env.observe_view(view_size=bad)
    G = 256                                                   # guard bytes on both sides of `out`
    buf = torch.zeros(G + n * 363 + G, dtype=torch.uint8, device=gpu)      # (room for the frames of the largest size)
    out = buf.data_ptr() + G
    assert out % 16 == 0
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    L, h = env.lib, env.handle
    assert L.bbai_observe_view(h, V, None, n, out + 1, stream) == -1            # BBAI_ERR_ARG: misaligned
    assert L.bbai_observe_view(h, V, None, n + 1, out, stream) == -1            # count > n without ids
    assert L.bbai_observe_view(h, 4, None, n, out, stream) == -1                # view sizes outside the five
    assert L.bbai_observe_view(h, 13, None, n, out, stream) == -1
    assert L.bbai_observe_view(None, V, None, n, out, stream) == -1             # null handle
    act = torch.zeros(n, dtype=torch.uint8, device=gpu)
    step_args = (act.data_ptr(), env.image.data_ptr(), env.direction.data_ptr(), env.reward.data_ptr(), env.reward64.data_ptr(),
                 env.done.data_ptr(), 1)
    assert L.bbai_step_view(h, *step_args, V, out + 8, stream) == -1
    assert L.bbai_step_view(h, *step_args, 6, out, stream) == -1
    fresh = make(gpu, level, seed=5, view_size=V)
    assert fresh.lib.bbai_observe_view(fresh.handle, V, None, n, out, stream) == -3       # BBAI_ERR_STATE: before reset
    fresh.close()
    torch.cuda.synchronize()
    assert not buf.any()                                      # nothing written by the refused calls
    # n * F bytes is not a multiple of 16: the tail of the whole batch goes out, and nothing past it or in front of it
    for v in (3, 5, 7, 9, 11):
        buf.zero_()
        assert L.bbai_observe_view(h, v, None, n, out, stream) == 0
        torch.cuda.synchronize()
        f = 3 * v * v
        assert torch.equal(buf[G:G + n * f].reshape(n, v, v, 3), env.observe_view(view_size=v, out=torch.empty((n, v, v, 3), dtype=torch.uint8, device=gpu)))
        assert not buf[:G].any() and not buf[G + n * f:].any(), v
    assert torch.equal(buf[G:G + n * 363].reshape(n, 11, 11, 3)[:, 5, 10], env.observe_view(view_size=3)[:, 1, 2])      # the agent's cell
    # a side stream
    side = torch.cuda.Stream(device=gpu)
    rng = np.random.RandomState(1)
    for t in range(3):
        env.step(torch.as_tensor(rng.randint(0, 7, size=n).astype(np.uint8), device=gpu))
        ids = np.arange(0, n, 7)
        torch.cuda.current_stream(gpu).synchronize()
        with torch.cuda.stream(side):
            fr = env.observe_view(ids)
        side.synchronize()
        assert torch.equal(fr, env.view[torch.as_tensor(ids, device=gpu)]), t
    env.close()


@pytest.mark.gpu
def test_expert_entries_refuse_a_view_size_batch(gpu):
    from babyai_amd.engine import EngineError
    env = make(gpu, "GoToLocal", n=8, view_size=5)
    env.reset()
    with pytest.raises(EngineError):
        env.bot_actions()
    with pytest.raises(EngineError):
        env.bot_rollout(4)
    env.close()


@pytest.mark.gpu
def test_parallel_env_adapter_and_device_rollout(gpu):
    """BatchedParallelEnv(view_size=5) hands out what a ParallelEnv loop over the oracle envs does (penv.py:8-11); DeviceRollout over a
    view_size=9 batch collects those frames; the preprocessor picks env.view."""
    import torch
    from babyai_amd.vec_env import BatchedParallelEnv
    from babyai_amd.rollout import DeviceRollout
    from rollout_util import ToyACModel
    level, P, seed = "GoToLocalS5N2", 24, 600
    venv = BatchedParallelEnv("BabyAI-%s-v0" % level, P, device=gpu, seeds=[seed + i for i in range(P)], view_size=5)
    refs = [oracle_env(level, seed + i, 5) for i in range(P)]
    assert venv.observation_space["image"].shape == (5, 5, 3)
    obss, wants = venv.reset(), [r.reset() for r in refs]
    rng = np.random.RandomState(0)
    for t in range(STEPS):
        for o, w in zip(obss, wants):
            assert set(o) == set(w) == {"image", "direction", "mission"}
            assert np.array_equal(o["image"], w["image"]) and o["mission"] == w["mission"] and o["direction"] == w["direction"], t
        acts = rng.randint(0, 7, size=P)
        obss, rew, done, _ = venv.step(acts)
        wants = []
        for r, a, rw, dn in zip(refs, acts, rew, done):
            o, rr, d, _ = r.step(int(a))
            assert (rr, d) == (rw, dn)
            wants.append(r.reset() if d else o)
    venv.close()

    T, V = 16, 9
    env = make(gpu, level, seed=seed, n=P, view_size=V)
    exps, _ = DeviceRollout(env, ToyACModel(), T, 0.99, 0.95).collect_experiences(copy=True)
    assert tuple(exps.obs.image.shape) == (P * T, V, V, 3)
    img = exps.obs.image.reshape(P, T, V, V, 3).to(torch.uint8).cpu().numpy()
    act = exps.action.reshape(P, T).cpu().numpy()
    for p in range(P):
        r = oracle_env(level, seed + p, V)
        o = r.reset()
        for t in range(T):
            assert np.array_equal(img[p, t], o["image"]), (p, t)
            o, _, d, _ = r.step(int(act[p, t]))
            if d:
                o = r.reset()
    env.close()


@pytest.mark.gpu
def test_kernel_resources_no_scratch_no_spills():
    with open(os.path.join(ROOT, "babyai_amd", "kernel_resources.json")) as f:
        kernels = json.load(f)["kernels"]
    names = ["k_view_obs<%d>" % v for v in (3, 5, 7, 9, 11)]
    for name in names:
        assert name in kernels, name
        assert kernels[name]["scratch_bytes_per_lane"] == 0 and kernels[name]["vgpr_spills"] == 0, (name, kernels[name])
    assert sorted(k for k in kernels if k.startswith("k_view_obs")) == sorted(names)
