"""The hold action on the device (include/bbai.h BBAI_ACTION_HOLD, option "step_hold"; step_body in babyai_amd/csrc/bbai_stepk.hpp): an env that
holds does not move, an env that steps goes exactly where it would have gone.  Envs are independent, so the reference is the engine's own
unheld run: batch A steps every env under a fixed action table a[t][i] and logs every output; batch B (same seeds) is stepped under a mask
schedule, env i taking its next unused action a[k_i][i] whenever it is not held.  After every call a stepped env's outputs must equal A's log at
(k_i, i) and a held env's must equal B's own from before the call.  130 envs: two full 64-env waves and a partial wave of 2, so the schedule
holds whole waves (they leave behind their action load), single lanes of stepping waves (the frozen arm) and everything in between."""
import numpy as np
import pytest

import render_util as ru

ROOM = "BabyAI-GoToLocal-v0"
BOSS = "BabyAI-BossLevel-v0"
N = 130
HOLD = 8
SEED = 4242
# case -> (level, variables set before create, options set after it, the layout the handle must report)
CASES = {
    "room": (ROOM, {}, {}, {"inplace": 1, "cplane": 1}),                          # in-place layout + C plane
    "maze": (BOSS, {}, {}, {"inplace": 0}),                                       # window plane, fused consume
    "maze_unfused": (BOSS, {}, {"consume_fused": 0}, {"inplace": 0}),             # ... finished envs listed for k_consume
    "room_classic": (ROOM, {"BBAI_INPLACE": "0"}, {}, {"inplace": 0, "cplane": 0}),
}
LAYOUT_VARS = ["BBAI_INPLACE", "BBAI_VPLANE", "BBAI_CPLANE", "BBAI_CONSUME_FUSED", "BBAI_LOOKAHEAD", "BBAI_ROLLOUT_MULTI"]
K = 160                # steps of batch A = steps every env of batch B ends with
CALLS = 320
RANDOM_END = 235       # calls 5 .. 234: independent p = 0.5 masks; from here on catch-up (everybody who is behind steps)
LONG, LONG_HOLD = 5, 100        # env 5 is held for 100 calls in a row in the middle of an episode
ENV_A, ENV_B, ENV_C, ENV_C_HELD = 3, 66, 67, 68     # the envs whose schedule is bent to contain the three named cases
_open = []


@pytest.fixture(autouse=True)
def _close_handles():
    yield
    while _open:
        _open.pop().close()


def make(gpu, monkeypatch, case, **kw):
    from babyai_amd.engine import BatchedBabyAIEnv
    level, variables, options, layout = CASES[case]
    for var in LAYOUT_VARS:
        monkeypatch.delenv(var, raising=False)
    for var, v in variables.items():
        monkeypatch.setenv(var, v)
    env = BatchedBabyAIEnv(level, N, device=gpu, seeds=SEED, **kw)
    _open.append(env)
    for name, v in options.items():
        env.set_option(name, v)
    for name, v in layout.items():
        assert env.get_option(name) == v, (case, name)
    return env


NAMES = ("image", "direction", "reward", "reward64 bits", "done")


def outputs(env):
    """The five output buffers on the host; reward64 as its bits."""
    return (env.image.cpu().numpy(), env.direction.cpu().numpy(), env.reward.cpu().numpy().view(np.uint32),
            env.reward64.cpu().numpy().view(np.uint64), env.done.cpu().numpy())


def action_table(seed, done_heavy=False):
    """a[t][i]: 0..6 at random with a RESET_ENV (7) in 3 % of the places -- the mazes' episodes outlast any test, so episodes end (and, under
    auto-reset, levels are consumed) because the table says so -- and at fixed places, which make the named cases certain.  done_heavy: the
    done-action mode's table, `done` (6) in 35 % of the places."""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 7, size=(K, N)).astype(np.uint8)
    if done_heavy:
        a = np.where(rng.rand(K, N) < 0.35, 6, rng.randint(0, 6, size=(K, N))).astype(np.uint8)
    a[rng.rand(K, N) < 0.03] = 7
    a[20, ENV_A] = a[30, ENV_B] = a[40, ENV_C] = a[90, LONG] = 7
    return a


def run_unheld(env, a, gpu):
    """Batch A: every env steps every action of its column; the log of every output per step, the final snapshot."""
    import torch
    env.reset()
    acts = torch.as_tensor(a, device=gpu)
    logs = []
    for t in range(len(a)):
        env.step(acts[t])
        logs.append(outputs(env))
    return [np.stack(x) for x in zip(*logs)], env.save_state()


def build_schedule(log, seed):
    """mask[c][i]: env i steps in call c.  Fixed, from A's log alone: the whole-batch hold, each wave held alone, one env alone, the random
    masks, the long hold of env LONG (it starts at the first call >= 20 that finds the env two steps into an episode), single holds placed
    where the named cases need them, and catch-up calls that bring every env to K steps."""
    done, rew = log[4], log[3].view(np.float64)
    rng = np.random.RandomState(seed)
    k = np.zeros(N, dtype=np.int64)
    masks, ks = [], []
    did, long_left, long_at, held_at_success = set(), None, None, set()
    for c in range(CALLS):
        m = np.ones(N, dtype=bool)
        if c == 0:
            m[:] = False
        elif c == 1:
            m[:64] = False
        elif c == 2:
            m[64:128] = False
        elif c == 3:
            m[128:] = False
        elif c == 4:
            m[:] = False
            m[70] = True
        elif c < RANDOM_END:
            m = rng.rand(N) < 0.5
            m[LONG] = True
            kl = k[LONG]
            if long_left is None and c >= 20 and kl >= 2 and not done[kl - 1, LONG] and not done[kl - 2, LONG]:
                long_left, long_at = LONG_HOLD, (c, int(kl))
            if long_left:
                m[LONG] = False
                long_left -= 1
            if "a" not in did and k[ENV_A] > 0 and done[k[ENV_A] - 1, ENV_A]:         # its last step ended an episode: held at step_count 0 / frozen
                m[ENV_A] = False
                did.add("a")
            if "b" not in did and k[ENV_B] < K and done[k[ENV_B], ENV_B]:              # its next step ends the episode
                m[ENV_B] = False
                did.add("b")
            if "c" not in did and m[ENV_C] and k[ENV_C] < K and done[k[ENV_C], ENV_C]:  # the lane next to it finishes in this call
                m[ENV_C_HELD] = False
                did.add("c")
            for i in range(N):                          # one hold in front of every rewarded step (of a live env: a frozen one repeats its reward)
                if k[i] < K and rew[k[i], i] > 0 and not (k[i] > 0 and done[k[i] - 1, i]) and (i, int(k[i])) not in held_at_success:
                    held_at_success.add((i, int(k[i])))
                    m[i] = False
        m &= k < K
        masks.append(m)
        ks.append(k.copy())
        k = k + m
    assert (k == K).all(), "the schedule does not bring every env to %d steps" % K
    return np.stack(masks), np.stack(ks), long_at


def named_cases(masks, ks, log):
    """How often the schedule holds an env (a) whose last step ended an episode, (b) whose next step ends one, (c) in a wave where another
    lane's step ends one, (d) whose next step is rewarded."""
    done, rew = log[4], log[3].view(np.float64)
    n = dict(a=0, b=0, c=0, d=0)
    idx = np.arange(N)
    for m, k in zip(masks, ks):
        held = ~m & (k < K)
        kk = np.minimum(k, K - 1)
        ends = (k < K) & (done[kk, idx] != 0)
        n["a"] += int((held & (k > 0) & (done[np.maximum(k, 1) - 1, idx] != 0)).sum())
        n["b"] += int((held & ends).sum())
        n["d"] += int((held & (k < K) & (rew[kk, idx] > 0) & ~((k > 0) & (done[np.maximum(k, 1) - 1, idx] != 0))).sum())
        for w in range(0, N, 64):
            if (m[w:w + 64] & ends[w:w + 64]).any():
                n["c"] += int((~m[w:w + 64]).sum())
    return n


def first_difference(got, want, held):
    for name, g, w in zip(NAMES, got, want):
        bad = np.nonzero((g != w).reshape(N, -1).any(axis=1))[0]
        if len(bad):
            return "%s of env %d (%s)" % (name, bad[0], "held" if held[bad[0]] else "stepped")
    return None


def run_masked(env, a, log, masks, gpu, long_at=None):
    """Batch B under the schedule, checked after every call; the three ways in take turns: step(ids=host list), step(ids=device tensor) and
    a full vector with HOLD bytes under the option.  Returns the step index at which env LONG's first episode end behind its long hold came."""
    import torch
    env.reset()
    prev = outputs(env)
    k = np.zeros(N, dtype=np.int64)
    long_end = None
    assert env.get_option("step_hold") == 0
    for c, m in enumerate(masks):
        ids = np.nonzero(m)[0]
        acts = a[k[ids], ids]
        if c % 3 == 0:
            env.step(acts, ids=ids)
        elif c % 3 == 1:
            env.step(torch.as_tensor(acts, device=gpu), ids=torch.as_tensor(ids, device=gpu))
        else:
            full = np.full(N, HOLD, dtype=np.uint8)
            full[ids] = acts
            env.set_option("step_hold", 1)
            env.step(torch.as_tensor(full, device=gpu))
            env.set_option("step_hold", 0)
        assert env.get_option("step_hold") == 0
        got = outputs(env)
        want = [p.copy() for p in prev]
        for w, l in zip(want, log):
            w[ids] = l[k[ids], ids]
        bad = first_difference(got, want, ~m)
        assert bad is None, "call %d: %s, k = %s" % (c, bad, k.tolist())
        if long_at is not None and long_end is None and c > long_at[0] and m[LONG] and got[4][LONG]:
            long_end = int(k[LONG])
        prev = got
        k = k + m
    assert (k == K).all()
    return long_end


def same_rows(x, y, rows=None):
    import torch
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])
    return all(torch.equal(pick(getattr(x, f)), pick(getattr(y, f))) for f in ("rec", "hot", "stale", "lsm"))


# ---- 1. the option by name (the test that fails without the feature: "unknown option") -------------------------------------------------
@pytest.mark.gpu
def test_the_option_by_name(gpu, monkeypatch):
    env = make(gpu, monkeypatch, "room")
    assert env.get_option("step_hold") == 0
    for v in (1, 5, -3):
        env.set_option("step_hold", v)
        assert env.get_option("step_hold") == 1              # FLAG: v != 0
    env.set_option("step_hold", 0)
    assert env.get_option("step_hold") == 0
    assert env.HOLD == HOLD


# ---- 2. off means off ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_with_the_option_off_byte_8_is_done(gpu, monkeypatch):
    import torch
    x, y = make(gpu, monkeypatch, "room"), make(gpu, monkeypatch, "room")
    x.reset()
    y.reset()
    rng = np.random.RandomState(1)
    n6 = 0
    for t in range(40):
        a6 = rng.randint(0, 7, size=N).astype(np.uint8)
        a8 = np.where(a6 == 6, 8, a6).astype(np.uint8)
        n6 += int((a6 == 6).sum())
        x.step(torch.as_tensor(a6, device=gpu))
        y.step(torch.as_tensor(a8, device=gpu))
        assert torch.equal(x.image, y.image) and torch.equal(x.reward64, y.reward64) and torch.equal(x.done, y.done), t
    assert n6 > 0 and int(x.reset_count()) == int(y.reset_count())


# ---- 3. + 8. held envs do not move, stepped envs go where they would have gone ------------------------------------------------------------
def masked_against_unheld(gpu, monkeypatch, case, table_seed, **kw):
    a = action_table(table_seed, done_heavy=bool(kw.get("done_actions")))
    A, B = make(gpu, monkeypatch, case, **kw), make(gpu, monkeypatch, case, **kw)
    log, snap_a = run_unheld(A, a, gpu)
    masks, ks, long_at = build_schedule(log, table_seed + 1)
    # the schedule contains what it was built to contain
    assert not masks[0].any() and (~masks[1]).nonzero()[0].tolist() == list(range(64)) and (~masks[2]).nonzero()[0].tolist() == list(range(64, 128))
    assert (~masks[3]).nonzero()[0].tolist() == [128, 129] and masks[4].nonzero()[0].tolist() == [70]
    assert sum(1 for m in masks if not m[:64].any() and m[64:].any()) > 0 and sum(1 for m in masks if not m.any()) > 0
    cases = named_cases(masks, ks, log)
    assert cases["a"] > 0 and cases["b"] > 0 and cases["c"] > 0, cases
    long_end = run_masked(B, a, log, masks, gpu, long_at)
    assert same_rows(B.save_state(), snap_a), "state rows after %d steps per env" % K
    assert A.gate_timeouts() == 0 and B.gate_timeouts() == 0
    assert int(A.reset_count()) == int(B.reset_count())
    return log, cases, long_at, long_end


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_masked_steps_against_the_unheld_run(gpu, monkeypatch, case):
    log, cases, long_at, long_end = masked_against_unheld(gpu, monkeypatch, case, 7)
    # 8.: env LONG sat out 100 calls in the middle of an episode (step long_at[1] of its column); that episode ends at the step it ends
    # at in A -- where the room's max_steps bound ends it, neither sooner (the holds were counted) nor later
    assert long_at is not None
    c0, k0 = long_at
    end_a = k0 + int(np.nonzero(log[4][k0:, LONG])[0][0])
    assert not log[4][k0 - 1, LONG] and long_end == end_a, (long_at, long_end, end_a)


@pytest.mark.gpu
def test_frozen_envs_stay_frozen_under_hold(gpu, monkeypatch):
    """auto_reset=False: an env that finished freezes; held or not it keeps re-emitting its last outputs (named case a = holds of frozen envs)."""
    masked_against_unheld(gpu, monkeypatch, "room", 11, auto_reset=False)


@pytest.mark.gpu
def test_a_hold_does_not_clear_last_step_match(gpu, monkeypatch):
    """Done-action mode: an instruction succeeds on a `done` right after the step that completed it.  The schedule holds every env once in
    front of each of its rewarded steps -- here between the completing step and the `done` -- and the reward of that `done` is A's."""
    log, cases, _, _ = masked_against_unheld(gpu, monkeypatch, "room", 13, done_actions=True)
    assert cases["d"] > 0, cases


# ---- 4. rollout under the option ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["room", "maze"])
def test_rollout_honours_hold_bytes_per_tick(gpu, monkeypatch, case):
    import torch
    T = 24
    rng = np.random.RandomState(3)
    a = rng.randint(0, 7, size=(T, N)).astype(np.uint8)
    a[rng.rand(T, N) < 0.05] = 7
    a[rng.rand(T, N) < 0.3] = HOLD
    a[3, :] = HOLD                      # a tick in which every wave leaves early
    a[5:10, 64:128] = HOLD              # ... and ticks in which one does
    a[12, :64] = HOLD
    a[12, 17] = 7
    acts = torch.as_tensor(a, device=gpu)
    R, S = make(gpu, monkeypatch, case), make(gpu, monkeypatch, case)
    for e in (R, S):
        e.reset()
        e.set_option("step_hold", 1)
    R.rollout(acts)
    for t in range(T):
        S.step(acts[t])
    assert torch.equal(R.image, S.image) and torch.equal(R.direction, S.direction)
    assert torch.equal(R.reward64, S.reward64) and torch.equal(R.done, S.done)
    assert same_rows(R.save_state(), S.save_state())
    assert int(R.reset_count()) == int(S.reset_count()) > N
    # ... and the held envs did hold: with the option off byte 8 is `done`, which moves nobody either but is a step that counts
    Z = make(gpu, monkeypatch, case)
    Z.reset()
    Z.rollout(acts)
    assert not torch.equal(Z.save_state().hot, R.save_state().hot)


# ---- 5. pixels ---------------------------------------------------------------------------------------------------------------------------
def pixel_masks(calls, seed):
    rng = np.random.RandomState(seed)
    masks = rng.rand(calls, N) < 0.5
    masks[3, :] = False
    masks[5, 64:128] = False
    masks[6, :64] = False
    masks[7, :] = False
    masks[7, 129] = True
    return masks


@pytest.mark.gpu
@pytest.mark.parametrize("tile_size,from_step", [(8, 1), (8, 0), (16, None)])
def test_pixels_follow_masked_steps(gpu, monkeypatch, tile_size, from_step):
    import torch
    env = make(gpu, monkeypatch, "room", pixel=True, tile_size=tile_size)
    if from_step is not None:
        env.set_option("render_delta_from_step", from_step)
    env.reset()
    rng = np.random.RandomState(5)
    for c, m in enumerate(pixel_masks(40, 6)):
        ids = np.nonzero(m)[0]
        acts = rng.randint(0, 7, size=len(ids)).astype(np.uint8)
        acts[rng.rand(len(ids)) < 0.05] = 7
        obs = env.step(acts, ids=ids)[0]
        assert obs["image"] is env.pixels
        assert torch.equal(env.pixels, env.render_encoding(env.image)), (tile_size, from_step, c)
    assert env.get_option("render_delta_valid") == 1


@pytest.mark.gpu
@pytest.mark.parametrize("from_step", [1, 0])
def test_a_held_wave_stores_no_pixel(gpu, monkeypatch, from_step):
    """The method of tests/test_gpu_render_delta_footprint.py: the frames of wave 1's envs are overwritten with their complement, without
    invalidating.  A call that holds the wave leaves those bytes the complement (from_step = 1: the wave that left early reported no dirty
    cell); a call that steps one of its envs stores exactly the pieces of that env's changed cells."""
    import torch
    env = make(gpu, monkeypatch, "room", pixel=True)
    env.set_option("render_delta_from_step", from_step)
    unit = env.get_option("render_piece_bytes")
    env.reset()
    rng = np.random.RandomState(9)
    for _ in range(3):
        env.step(torch.as_tensor(rng.randint(0, 3, size=N).astype(np.uint8), device=gpu))
    assert env.get_option("render_delta_valid") == 1
    px = env.pixels.view(N, -1)
    comp = 255 - px[64:128]
    px[64:128] = comp
    others = np.r_[0:64, 128:N]
    env.step(rng.randint(0, 3, size=len(others)).astype(np.uint8), ids=others)
    assert torch.equal(px[64:128], comp), "a held wave's frames were stored"
    whole = env.render_encoding(env.image).view(N, -1)
    assert torch.equal(px[torch.as_tensor(others, device=gpu)], whole[torch.as_tensor(others, device=gpu)])
    before, old_ids = px.cpu().numpy().reshape(-1), ru.tile_ids(env.image.cpu().numpy())
    env.step([0], ids=[70])                                   # a turn: the whole view changes
    new_ids = ru.tile_ids(env.image.cpu().numpy())
    mask = ru.stored_mask(old_ids, new_ids, unit)
    per_env = mask.reshape(N, -1)
    assert per_env[70].any() and not per_env[70].all() and not np.delete(per_env, 70, axis=0).any()
    want = np.where(mask, ru.frames(new_ids).reshape(-1), before)
    got = px.cpu().numpy().reshape(-1)
    assert np.array_equal(got, want), "bytes off: %d inside the pieces to store, %d outside" % (int((got != want)[mask].sum()), int((got != want)[~mask].sum()))


# ---- 6. full observations and the tap ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_full_observations_follow_masked_steps(gpu, monkeypatch):
    import torch
    env = make(gpu, monkeypatch, "room", full_obs=True)
    env.reset()
    rng = np.random.RandomState(15)
    for c, m in enumerate(pixel_masks(20, 16)):
        ids = np.nonzero(m)[0]
        obs = env.step(rng.randint(0, 7, size=len(ids)).astype(np.uint8), ids=ids)[0]
        assert obs["image"] is env.full
        assert torch.equal(env.full, env.observe_full(out=torch.empty_like(env.full))), c


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["room", "maze", "maze_unfused"])
def test_the_tap_logs_held_envs_unchanged(gpu, monkeypatch, case):
    """step_tapped with holds: one row per listed env per step -- the new outputs of a listed env that stepped, the unchanged ones of one
    that held.  Env 65 is listed and, in calls 2, 3 and 6, sits in a wave that is otherwise (and itself) entirely held."""
    import torch
    listed = [129, 2, 65]
    a = action_table(21)
    A, B = make(gpu, monkeypatch, case), make(gpu, monkeypatch, case)
    log, _ = run_unheld(A, a[:40], gpu)
    B.reset()
    B.set_step_tap(listed)
    B.set_option("step_hold", 1)
    rng = np.random.RandomState(22)
    masks = rng.rand(30, N) < 0.6
    masks[2, 64:128] = masks[3, 64:128] = masks[6, 64:128] = False
    masks[4, :] = False
    rows = (torch.zeros((3, 7, 7, 3), dtype=torch.uint8, device=gpu), torch.zeros((3,), dtype=torch.uint8, device=gpu),
            torch.zeros((3,), dtype=torch.float64, device=gpu), torch.zeros((3,), dtype=torch.uint8, device=gpu))
    prev, k = outputs(B), np.zeros(N, dtype=np.int64)
    for c, m in enumerate(masks):
        ids = np.nonzero(m)[0]
        full = np.full(N, HOLD, dtype=np.uint8)
        full[ids] = a[k[ids], ids]
        for r in rows:
            r.fill_(77)
        B.step_tapped(torch.as_tensor(full, device=gpu), *rows)
        got = outputs(B)
        want = [p.copy() for p in prev]
        for w, l in zip(want, log):
            w[ids] = l[k[ids], ids]
        bad = first_difference(got, want, ~m)
        assert bad is None, "call %d: %s" % (c, bad)
        assert np.array_equal(rows[0].cpu().numpy(), got[0][listed]), c
        assert np.array_equal(rows[1].cpu().numpy(), got[1][listed]), c
        assert np.array_equal(rows[2].cpu().numpy().view(np.uint64), got[3][listed]), c
        assert np.array_equal(rows[3].cpu().numpy(), got[4][listed]), c
        prev, k = got, k + m
    assert B.gate_timeouts() == 0


# ---- 7. lookahead --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case,on_device", [("room", True), ("maze", False)])
def test_lookahead_expands_the_listed_states_and_moves_nobody_else(gpu, monkeypatch, case, on_device):
    import torch
    roots = [1, 64, 70, 128, 129]
    scratch = list(range(40, 60)) + list(range(100, 115))             # 35 envs of waves 0 and 1
    L, T = make(gpu, monkeypatch, case), make(gpu, monkeypatch, case)
    rng = np.random.RandomState(31)
    for e in (L, T):
        e.reset()
    for t in range(10):
        act = torch.as_tensor(rng.randint(0, 7, size=N).astype(np.uint8), device=gpu)
        L.step(act)
        T.step(act)
    others = torch.as_tensor(sorted(set(range(N)) - set(scratch)), device=gpu)
    before, image_before = L.save_state(), L.image.clone()
    dev = lambda ids: torch.as_tensor(ids, dtype=torch.int64, device=gpu)
    out = L.lookahead(dev(roots), dev(scratch)) if on_device else L.lookahead(roots, scratch)
    assert same_rows(L.save_state(), before, others), "lookahead moved an env that is not a scratch env"
    assert torch.equal(L.image[others], image_before[others])
    assert L.get_option("step_hold") == 0
    assert tuple(out["image"].shape) == (5, 7, 7, 7, 3) and all(tuple(out[f].shape) == (5, 7) for f in ("direction", "reward", "reward64", "done"))
    # the twin: the same history, stepped once per action from a restored snapshot
    snap = T.save_state()
    compared = 0
    for action in range(7):
        T.load_state(snap)
        T.step(torch.full((N,), action, dtype=torch.uint8, device=gpu))
        for j, r in enumerate(roots):
            assert out["reward64"][j, action].item() == T.reward64[r].item() and out["done"][j, action].item() == T.done[r].item(), (j, action)
            assert out["reward"][j, action].item() == T.reward[r].item()
            if not T.done[r].item():          # (a child whose episode ended shows the scratch env's own next level, the twin the root's)
                assert torch.equal(out["image"][j, action], T.image[r]) and out["direction"][j, action].item() == T.direction[r].item(), (j, action)
                compared += 1
    assert compared >= 30
