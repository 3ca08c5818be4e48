"""Device snapshots (k_state_save / k_state_load, include/bbai.h bbai_save_state / bbai_load_state): the format is export_state's, a
rewind replays bit for bit (also in done-action mode, where the lastStepMatch byte decides), a loaded env behaves as one that got the same
state through the host import, nothing but the listed envs moves -- their own level streams included --, the start-carry levels give
gen_obs() of the state after the hand-over, every observation kind follows, token rows and the expert follow, and the edges hold."""
import numpy as np
import pytest

N = 192
LEVELS = ["GoToLocal", "BossLevel", "PutNextS5N2Carrying"]
VARIANTS = [(lv, {"BBAI_INPLACE": ip}) for lv in LEVELS for ip in ("0", "1")] + \
    [("GoToLocal", {"BBAI_INPLACE": "0", "BBAI_VPLANE": "0"}), ("GoToLocal", {"BBAI_INPLACE": "1", "BBAI_CPLANE": "0"})]
VIDS = ["%s-%s" % (lv, "-".join("%s%s" % (k[5:].lower(), v) for k, v in sorted(ev.items()))) for lv, ev in VARIANTS]
KEYS = ("image", "direction", "reward", "reward64", "done")


def _setenv(monkeypatch, ev):
    for k, v in ev.items():
        monkeypatch.setenv(k, v)


def _make(level, n, gpu, seed, **kw):
    from babyai_amd.engine import BatchedBabyAIEnv
    env = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device=gpu, seeds=seed, **kw)
    env.reset()
    return env


def _ids37(n, seed=3):
    """37 envs that include 0 and n - 1 and both sides of every 64-env boundary, in no order."""
    edge = [0, n - 1] + [b + d for b in range(64, n, 64) for d in (-1, 0) if 0 < b + d < n - 1]
    rng = np.random.RandomState(seed)
    rest = [i for i in rng.permutation(n) if i not in edge]
    ids = np.array(edge + rest[:37 - len(edge)], dtype=np.int64)
    assert len(ids) == 37 and len(set(ids.tolist())) == 37
    return rng.permutation(ids)


def _acts(gpu, T, n, seed):
    import torch
    return torch.as_tensor(np.random.RandomState(seed).randint(0, 7, size=(T, n)).astype(np.uint8), device=gpu)


def _run(env, acts, extra=()):
    """Step through acts[T, n]; every output of every step, stacked on the device."""
    import torch
    out = {k: [] for k in KEYS + tuple(extra)}
    for t in range(acts.shape[0]):
        env.step(acts[t])
        for k in KEYS:
            out[k].append(getattr(env, k).clone())
        for k in extra:
            out[k].append(getattr(env, k).clone())
    return {k: torch.stack(v) for k, v in out.items()}


def _assert_same(a, b, cols_a=None, cols_b=None, keys=KEYS, what=""):
    import torch
    for k in keys:
        x = a[k] if cols_a is None else a[k][:, cols_a]
        y = b[k] if cols_b is None else b[k][:, cols_b]
        if not torch.equal(x, y):
            bad = (x != y).reshape(x.shape[0], x.shape[1], -1).any(-1).nonzero()[:6].tolist()
            raise AssertionError("%s %s differs at (step, column) %s" % (what, k, bad))


def _snap_np(snap):
    return snap.rec.cpu().numpy(), snap.hot.cpu().numpy(), snap.stale.cpu().numpy().view(np.uint64), snap.lsm.cpu().numpy()


# ---- 1. format ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("level,ev,n", [(lv, ev, N) for lv, ev in VARIANTS] + [("GoToLocal", {"BBAI_INPLACE": "1"}, 65), ("BossLevel", {"BBAI_INPLACE": "0"}, 65)],
                         ids=VIDS + ["GoToLocal-n65", "BossLevel-n65"])
def test_rows_are_export_states_rows(gpu, monkeypatch, level, ev, n):
    import torch
    _setenv(monkeypatch, ev)
    env = _make(level, n, gpu, 300)
    _run(env, _acts(gpu, 20, n, 1))
    ids = _ids37(n)
    rec, hot, stale = env.export_state()
    for which, sel in ((ids, ids), (torch.as_tensor(ids, device=gpu), ids), (None, np.arange(n))):
        snap = env.save_state(which)
        assert len(snap) == len(sel) and snap.rec_bytes == env.cfg.rec_bytes and snap.env_id == level and snap.done_actions is False
        srec, shot, sstale, slsm = _snap_np(snap)
        assert np.array_equal(srec, rec[sel]) and np.array_equal(shot, hot[sel]) and np.array_equal(sstale, stale[sel])
        assert not slsm.any()
    env.close()


# ---- 2. rewind ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("level,ev,n", [(lv, ev, N) for lv, ev in VARIANTS] + [("GoToLocal", {"BBAI_INPLACE": "1"}, 65), ("GoToLocal", {"BBAI_INPLACE": "0"}, 65)],
                         ids=VIDS + ["GoToLocal-inplace1-n65", "GoToLocal-inplace0-n65"])
def test_rewind_replays_every_output(gpu, monkeypatch, level, ev, n):
    import torch
    _setenv(monkeypatch, ev)
    env = _make(level, n, gpu, 420, auto_reset=False)
    _run(env, _acts(gpu, 20, n, 2))
    snap = env.save_state()
    image0, dir0 = env.image.clone(), env.direction.clone()
    acts = _acts(gpu, 40, n, 3)
    first = _run(env, acts)
    obs = env.load_state(snap)
    assert obs["image"] is env.image
    assert torch.equal(obs["image"], image0) and torch.equal(obs["direction"], dir0)
    again = _run(env, acts)
    _assert_same(first, again, what="replay")
    if level == "GoToLocal":
        assert bool(first["done"][-1].any())          # (envs froze on the way: they are part of the comparison)
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", ["0", "1"])
def test_rewind_in_done_action_mode_needs_last_step_match(gpu, monkeypatch, inplace):
    """GoToLocal under BABYAI_DONE_ACTIONS: `done` succeeds only right after the step that brought the agent in front of its target, and ends the
    episode in failure at any other time -- so the random steps here draw from the six other actions.  The replay starts with `done` for the envs
    saved in that position: they earn their reward again only if their lastStepMatch byte came back."""
    import torch
    monkeypatch.setenv("BBAI_INPLACE", inplace)
    env = _make("GoToLocal", N, gpu, 77, auto_reset=False, done_actions=True)
    pre = _acts(gpu, 45, N, 4) % 6
    snap = None
    for t in range(45):          # 20 random steps, then on until some env stands in front of its target (one object of nine, 36 cells: a few of 192 do after any step)
        env.step(pre[t])
        if t >= 19:
            snap = env.save_state()
            if bool(((snap.lsm != 0) & (snap.hot[:, 13] == 0)).any()):
                break
    matched = (snap.lsm != 0) & (snap.hot[:, 13] == 0)          # (Hot.frozen: a finished env takes no action)
    assert bool(matched.any()), "no env stood in front of its target in 45 steps: choose other seeds"
    assert snap.done_actions
    image0, dir0 = env.image.clone(), env.direction.clone()
    acts = _acts(gpu, 40, N, 5) % 6
    acts[0][matched] = 6
    acts[7] = 6                  # ... and `done` for everyone later on: it succeeds or fails by the byte as the replay left it
    first = _run(env, acts)
    assert bool((first["reward64"][0][matched] > 0).all()), "`done` right after the matching step must succeed"
    obs = env.load_state(snap)
    assert torch.equal(obs["image"], image0) and torch.equal(obs["direction"], dir0)
    again = _run(env, acts)
    _assert_same(first, again, what="done-action replay")
    # the same snapshot without its lastStepMatch bytes is another state: those envs' `done` fails
    from babyai_amd.engine import EnvSnapshot
    env.load_state(EnvSnapshot(snap.rec, snap.hot, snap.stale, torch.zeros_like(snap.lsm), snap.env_id, snap.rec_bytes, True))
    env.step(acts[0])
    assert bool((env.reward64[matched] == 0).all())
    env.close()


# ---- 3. pinned to the host import -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("level,ev,ev_src", [(lv, ev, ev) for lv, ev in VARIANTS] + [("GoToLocal", {"BBAI_INPLACE": "1"}, {"BBAI_INPLACE": "0"}),
                                                                                    ("BossLevel", {"BBAI_INPLACE": "0"}, {"BBAI_INPLACE": "1"})],
                         ids=VIDS + ["GoToLocal-classic-to-inplace", "BossLevel-inplace-to-classic"])
def test_loaded_envs_behave_as_host_imported_ones(gpu, monkeypatch, level, ev, ev_src):
    import torch
    _setenv(monkeypatch, ev_src)
    src = _make(level, N, gpu, 100)
    _run(src, _acts(gpu, 20, N, 6))
    snap = src.save_state()
    rec, hot, stale = src.export_state()
    _setenv(monkeypatch, ev)
    ids = _ids37(N, seed=8)
    rng = np.random.RandomState(9)
    rows = np.concatenate([np.full(7, 5), rng.choice(np.setdiff1d(np.arange(N), [5]), 30, replace=False)]).astype(np.int64)   # row 5 into seven envs
    h2 = _make(level, N, gpu, 7000, auto_reset=False)
    h3 = _make(level, 37, gpu, 9000, auto_reset=False)
    obs = h2.load_state(snap, ids=ids, rows=torch.as_tensor(rows, device=gpu))
    h3.import_state(rec[rows], hot[rows], stale[rows])
    fresh = torch.as_tensor(src.done.cpu().numpy()[rows] == 0, device=gpu)       # (a row that has just auto-reset shows reset()'s observation: start-carry levels)
    tids, trows = torch.as_tensor(ids, device=gpu), torch.as_tensor(rows, device=gpu)
    assert torch.equal(obs["image"][tids][fresh], src.image[trows][fresh]) and torch.equal(obs["direction"][tids][fresh], src.direction[trows][fresh])
    a3 = _acts(gpu, 30, 37, 10)
    a3[0, :7] = torch.arange(7, dtype=torch.uint8, device=gpu)                  # the seven copies: one action each
    a2 = _acts(gpu, 30, N, 11)
    a2[:, tids] = a3
    out2, out3 = _run(h2, a2), _run(h3, a3)
    _assert_same(out2, out3, cols_a=tids, keys=("image", "direction", "reward64", "done"), what="loaded vs imported")
    for h in (src, h2, h3):
        h.close()


# ---- 4. nothing else moves ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("inplace", ["0", "1"])
def test_other_envs_and_the_level_streams_stay(gpu, monkeypatch, inplace):
    """GoToLocal episodes last 64 steps at most, so in 200 steps behind the load every env starts three new episodes at least, in both batches."""
    import torch
    monkeypatch.setenv("BBAI_INPLACE", inplace)
    monkeypatch.setenv("BBAI_LOOKAHEAD", "4")
    a, b = _make("GoToLocal", N, gpu, 1234), _make("GoToLocal", N, gpu, 1234)
    for h in (a, b):
        h.enable_instr_tokens()
    pre = _acts(gpu, 25, N, 12)
    _run(a, pre[:10]); _run(b, pre[:10])
    snap = a.save_state()
    _run(a, pre[10:]); _run(b, pre[10:])
    assert torch.equal(a.image, b.image)
    ids = _ids37(N, seed=13)
    rows = np.random.RandomState(14).choice(N, 37, replace=False)
    a.load_state(snap, ids=ids, rows=rows)
    acts = _acts(gpu, 200, N, 15)
    oa, ob = _run(a, acts, extra=("instr",)), _run(b, acts, extra=("instr",))
    unl = torch.as_tensor(np.setdiff1d(np.arange(N), ids), device=gpu)
    _assert_same(oa, ob, cols_a=unl, cols_b=unl, keys=KEYS + ("instr",), what="unlisted env")
    da, db = oa["done"].cpu().numpy() != 0, ob["done"].cpu().numpy() != 0
    assert a.reset_count() - b.reset_count() == int(da.sum()) - int(db.sum())
    ia, ib, ta, tb = (x.cpu().numpy() for x in (oa["image"], ob["image"], oa["instr"], ob["instr"]))
    differ = 0
    for i in ids:
        sa, sb = np.nonzero(da[:, i])[0], np.nonzero(db[:, i])[0]          # the steps that started a new episode
        m = min(len(sa), len(sb))
        assert m >= 2, (i, len(sa), len(sb))
        differ += int(not np.array_equal(sa[:m], sb[:m]))
        for j in range(m):
            assert np.array_equal(ia[sa[j], i], ib[sb[j], i]), ("first observation of later episode", i, j)
            assert np.array_equal(ta[sa[j], i], tb[sb[j], i]), ("mission of later episode", i, j)
    assert differ > 0           # (the loaded episodes did run differently from the twin's)
    assert a.gate_timeouts() == 0 and b.gate_timeouts() == 0
    a.close(); b.close()


# ---- 5. start-carry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("inplace", ["0", "1"])
def test_start_carry_snapshot_is_the_state_after_the_hand_over(gpu, monkeypatch, inplace):
    import torch
    from test_gpu_parity import _oracle_envs
    monkeypatch.setenv("BBAI_INPLACE", inplace)
    seed = 600
    env = _make("PutNextS5N2Carrying", N, gpu, seed, auto_reset=False)
    reset_image = env.image.clone()
    snap = env.save_state()
    dst = _ids37(N, seed=16)
    srcs = np.random.RandomState(17).choice(np.setdiff1d(np.arange(N), dst), 37, replace=False)
    obs = env.load_state(snap, ids=dst, rows=srcs)
    got = obs["image"].cpu().numpy()
    refs = _oracle_envs("PutNextS5N2Carrying", [seed + int(s) for s in srcs])
    moved = 0
    for k, r in enumerate(refs):
        first = r.reset()["image"]
        want = r.gen_obs()["image"]
        assert r.carrying is not None
        assert np.array_equal(got[dst[k]], want), (k, int(dst[k]), int(srcs[k]))
        moved += int(not np.array_equal(first, want))
    assert moved > 0                                     # (the carried object's cell and the agent's: not what reset() returned)
    unl = torch.as_tensor(np.setdiff1d(np.arange(N), dst), device=gpu)
    assert torch.equal(obs["image"][unl], reset_image[unl])
    a = _acts(gpu, 1, N, 18)
    a[0, torch.as_tensor(dst, device=gpu)] = a[0, torch.as_tensor(srcs, device=gpu)]
    out = _run(env, a)
    _assert_same(out, out, cols_a=torch.as_tensor(dst, device=gpu), cols_b=torch.as_tensor(srcs, device=gpu), what="first step of the loaded env vs its source")
    env.close()


# ---- 6. observation kinds --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["pixel8", "pixel16", "full"])
@pytest.mark.parametrize("level", ["GoToLocal", "BossLevel"])
def test_every_observation_kind_follows_a_load(gpu, level, kind):
    import torch
    kw = {"pixel8": dict(pixel=True, tile_size=8), "pixel16": dict(pixel=True, tile_size=16), "full": dict(full_obs=True)}[kind]
    env = _make(level, N, gpu, 800, **kw)

    def fresh():
        if kind == "full":
            return env.observe_full(out=torch.zeros_like(env.full))
        return env.render_encoding(env.image, out=torch.zeros_like(env.pixels))

    acts = _acts(gpu, 38, N, 19)
    _run(env, acts[:20])
    snap = env.save_state()
    _run(env, acts[20:35])
    ids = _ids37(N, seed=20)
    obs = env.load_state(snap, ids=ids, rows=ids)
    assert obs["image"] is (env.full if kind == "full" else env.pixels)
    assert torch.equal(obs["image"], fresh()), "after load_state"
    rec, hot, _ = env.export_state()
    assert np.array_equal(rec[ids], snap.rec.cpu().numpy()[ids])
    for t in range(35, 38):
        obs, _, _, _ = env.step(acts[t])
        assert torch.equal(obs["image"], fresh()), ("step", t)
    env.close()


# ---- 7. tokens and the expert ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("level,inplace", [("GoToLocal", "0"), ("GoToLocal", "1"), ("BossLevel", "0")])
def test_token_rows_and_a_fresh_expert(gpu, monkeypatch, level, inplace):
    """The expected decisions come from a host import into a handle that never consulted the expert; what an import does to a handle that did
    is tests/test_gpu_state_ranges.py::test_an_import_starts_a_fresh_expert's."""
    import torch
    monkeypatch.setenv("BBAI_INPLACE", inplace)
    src = _make(level, N, gpu, 100)
    src.enable_instr_tokens()
    _run(src, _acts(gpu, 10, N, 21))
    snap = src.save_state()
    rec, hot, stale = src.export_state()
    b = _make(level, N, gpu, 5000)
    b.enable_instr_tokens()
    prev = None
    for t in range(10):              # the expert on every env: its plans expect step 10 next -- the step most loaded states are at
        act = b.bot_actions(prev).clone()
        act[act == b.BOT_GAVE_UP] = 6
        b.step(act)
        prev = act
    before = b.instr.clone()
    ids = _ids37(N, seed=22)
    rows = np.random.RandomState(23).choice(N, 37, replace=True).astype(np.int64)
    b.load_state(snap, ids=ids, rows=rows)
    tids, trows = torch.as_tensor(ids, device=gpu), torch.as_tensor(rows, device=gpu)
    assert torch.equal(b.instr[tids], src.instr[trows])
    unl = torch.as_tensor(np.setdiff1d(np.arange(N), ids), device=gpu)
    assert torch.equal(b.instr[unl], before[unl])
    assert not torch.equal(b.instr[tids], before[tids])
    assert int((snap.hot[trows, 4].to(torch.int32) | (snap.hot[trows, 5].to(torch.int32) << 8)).eq(10).sum()) >= 20      # Hot.step of the loaded rows
    got = b.bot_actions()[tids].cpu().numpy()
    c = _make(level, 37, gpu, 6000)
    c.import_state(rec[rows], hot[rows], stale[rows])
    want = c.bot_actions().cpu().numpy()
    assert np.array_equal(got, want), np.nonzero(got != want)[0].tolist()
    for h in (src, b, c):
        h.close()


# ---- 8. edges ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("inplace", ["0", "1"])
def test_empty_lists_and_ids_outside_the_batch(gpu, monkeypatch, inplace):
    import torch
    monkeypatch.setenv("BBAI_INPLACE", inplace)
    env = _make("GoToLocal", N, gpu, 900)
    _run(env, _acts(gpu, 12, N, 24))
    snap = env.save_state()
    _run(env, _acts(gpu, 9, N, 25))
    rec0, hot0, stale0 = env.export_state()
    image0 = env.image.clone()
    assert len(env.save_state([])) == 0
    obs = env.load_state(snap.select([]), ids=[], rows=[])
    rec1, hot1, stale1 = env.export_state()
    assert np.array_equal(rec0, rec1) and np.array_equal(hot0, hot1) and np.array_equal(stale0, stale1) and torch.equal(obs["image"], image0)
    # -1 and N inside a list: skipped; their neighbours are loaded
    ids = np.array([5, -1, 70, N, 130, 191], dtype=np.int64)
    rows = np.array([3, 4, 5, 6, 7, 8], dtype=np.int64)
    bad = env.save_state(ids)
    brec, bhot, bstale, _ = _snap_np(bad)
    ok = (ids >= 0) & (ids < N)
    assert np.array_equal(brec[ok], rec0[ids[ok]]) and not brec[~ok].any() and not bhot[~ok].any()
    obs = env.load_state(snap, ids=torch.as_tensor(ids, device=gpu), rows=torch.as_tensor(rows, device=gpu))
    rec2, hot2, stale2 = env.export_state()
    srec, shot, sstale, _ = _snap_np(snap)
    others = np.setdiff1d(np.arange(N), ids[ok])
    assert np.array_equal(rec2[others], rec0[others]) and np.array_equal(hot2[others], hot0[others]) and np.array_equal(stale2[others], stale0[others])
    assert torch.equal(obs["image"][torch.as_tensor(others, device=gpu)], image0[torch.as_tensor(others, device=gpu)])
    assert np.array_equal(rec2[ids[ok]], srec[rows[ok]]) and np.array_equal(stale2[ids[ok]], sstale[rows[ok]])
    assert np.array_equal(hot2[ids[ok], :15], shot[rows[ok], :15]) and np.array_equal(hot2[ids[ok], 15], hot0[ids[ok], 15])      # the env keeps its ring slot
    # a row outside the snapshot is skipped as well
    env.load_state(snap, ids=torch.as_tensor([9, 10], device=gpu), rows=torch.as_tensor([N, -1], device=gpu))
    rec3, _, _ = env.export_state()
    assert np.array_equal(rec3, rec2)
    env.close()


@pytest.mark.gpu
def test_a_call_on_another_stream_is_ordered_with_the_step_behind_it(gpu):
    import torch
    x, y = _make("GoToLocal", N, gpu, 950), _make("GoToLocal", N, gpu, 950)
    pre = _acts(gpu, 12, N, 26)
    a = _acts(gpu, 2, N, 27)
    ids = torch.as_tensor(_ids37(N, seed=28), device=gpu)
    rows = torch.as_tensor(np.random.RandomState(29).choice(N, 37), device=gpu)
    snaps = []
    for h in (x, y):
        _run(h, pre[:6])
        snaps.append(h.save_state())
        _run(h, pre[6:])
    x.load_state(snaps[0], ids=ids, rows=rows)
    ox = _run(x, a)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        y.load_state(snaps[1], ids=ids, rows=rows)
        oy = _run(y, a)          # (no synchronisation between the load and the steps)
    side.synchronize()
    _assert_same(ox, oy, what="default stream vs another")
    x.close(); y.close()
