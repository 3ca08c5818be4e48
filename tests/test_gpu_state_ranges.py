"""bbai_export_state / bbai_import_state / bbai_get_programs on env RANGES (first, count), against the host build: the index arithmetic of
k_live_copy, k_import_hot, k_sync_prog, k_sync_view and k_sync_cpl (bbai_ring.hpp) and of the host side's copies, in every state layout.  A
range export is a slice of the whole-batch export, which is the host model's state, and disturbs nothing; an import into a range of a live,
auto-resetting batch leaves every env stepping as the host model does -- the imported envs in the donor rows' episodes and then in their OWN
next levels, the others as an undisturbed twin --; imports without records move poses only; done-action mode starts with a cleared
lastStepMatch; pixels, the registered token rows and the expert follow the imported records; the edges hold.  Exact equality throughout,
rewards by bit pattern.  The scripts and what they reach are built on the host model alone (tests/state_ranges_util.py; pinned without a GPU
by tests/test_scenario_host.py).  BBAI_LOOKAHEAD=4 throughout."""
import numpy as np
import pytest

import scenario_util as su
import state_ranges_util as sr
from test_gpu_state_snapshot import VARIANTS, VIDS

N, B, RANGES = sr.N, sr.B, sr.RANGES
G, BOSS = "GoToLocal", "BossLevel"
IP0, IP1 = {"BBAI_INPLACE": "0"}, {"BBAI_INPLACE": "1"}
LAYOUTS = [(lv, ev, False) for lv, ev in VARIANTS] + [(G, IP0, True), (G, IP1, True)]
LIDS = VIDS + ["GoToLocal-done-inplace0", "GoToLocal-done-inplace1"]
RIDS = ["%d+%d" % r for r in RANGES]


@pytest.fixture(autouse=True)
def _short_windows(monkeypatch):
    monkeypatch.setenv("BBAI_LOOKAHEAD", str(B))


def _make(gpu, monkeypatch, level, ev, base, done_actions=False, tokens=False, n=N, **kw):
    from babyai_amd.engine import BatchedBabyAIEnv
    for k, v in ev.items():
        monkeypatch.setenv(k, v)
    env = BatchedBabyAIEnv("BabyAI-%s-v0" % level, n, device=gpu, seeds=sr.seeds(base, n), done_actions=done_actions, **kw)
    assert env.get_option("inplace") == int(ev["BBAI_INPLACE"]) and env.get_option("lookahead_period") == B
    if "BBAI_CPLANE" in ev:
        assert env.get_option("cplane") == int(ev["BBAI_CPLANE"])
    assert env.get_option("done_action_enum") == 0          # (the models below run with enum_done=False)
    if tokens:
        env.enable_instr_tokens()
    env.reset()
    return env


def _dev(gpu, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=gpu)


def _steps(env, acts):
    for a in acts:
        env.step(a)


def _state_equals(what, env, rows, first=0):
    rec, hot, stale = env.export_state()
    k = len(rows["stale"])
    su._same(what + " records", rec[first:first + k], rows["rec"])
    su._same(what + " hot bytes 0..14", hot[first:first + k, :15], rows["hot"][:, :15])          # (byte 15: the env's place in its own ring)
    su._same(what + " stale sets", stale[first:first + k], rows["stale"])


def _outside_equal_twin(got, twin, first, count):
    out = np.setdiff1d(np.arange(N), np.arange(first, first + count))
    for k, rows in got["steps"].items():
        for t, row in enumerate(rows):
            su._same("step %d %s of the envs outside the range vs the twin" % (t, k), row[out], twin["steps"][k][t][out])


def _finish(env, starts=None):
    assert env.get_option("gate_timeouts") == 0 and env.generator_failures() == 0
    if starts is not None:
        assert env.reset_count() == starts, (env.reset_count(), starts)
    env.close()


def _donor(gpu, monkeypatch, level, ev, done_actions=False, tokens=False):
    """The device donor of sr.donor: its whole-batch export is the model's state (asserted), so the model's scripts hold its rows."""
    d = _make(gpu, monkeypatch, level, ev, sr.DONOR_SEED, done_actions, tokens)
    _steps(d, _dev(gpu, sr.donor_acts()))
    _state_equals("donor", d, sr.state_rows(sr.donor(level, done_actions)))
    return d


# ---- 1. a range export is a slice and disturbs nothing ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("level,ev,done_actions", LAYOUTS, ids=LIDS)
def test_range_export_is_a_slice_and_disturbs_nothing(gpu, monkeypatch, level, ev, done_actions):
    import torch
    acts = _dev(gpu, su._acts(40, N, 90, 0.0))
    a, b = (_make(gpu, monkeypatch, level, ev, 300, done_actions) for _ in range(2))
    _steps(a, acts[:20]); _steps(b, acts[:20])
    m = sr.stepped_model(level, 300, su._acts(40, N, 90, 0.0)[:20], done_actions)
    rec, hot, stale = a.export_state()
    prog = a.programs()
    grid, pose = a.grid_encoding()
    want = sr.state_rows(m)
    su._same("records", rec, want["rec"]); su._same("hot bytes 0..14", hot[:, :15], want["hot"][:, :15]); su._same("stale sets", stale, want["stale"])
    su._same("programs", prog, want["rec"][:, a.cfg.off_prog:a.cfg.off_prog + prog.shape[1]])
    for first, count in RANGES:
        r, h, s = a.export_state(first, count)
        assert r.shape == (count, a.cfg.rec_bytes) and h.shape == (count, 16) and s.shape == (count,)
        sl = slice(first, first + count)
        assert np.array_equal(r, rec[sl]) and np.array_equal(h, hot[sl]) and np.array_equal(s, stale[sl]), (first, count)
        if count:          # (bbai_get_programs takes no NULL buffer, and a zero-size array's pointer may be one)
            assert np.array_equal(a.programs(first, count), prog[sl]), (first, count)
        g, p = a.grid_encoding(first, count)
        assert np.array_equal(g, grid[sl]) and np.array_equal(p, pose[sl]), (first, count)
    for t in range(20, 40):          # the in-place layout's exports wrote the staging area: the twin never exported
        a.step(acts[t]); b.step(acts[t])
        for k in ("image", "direction", "reward", "reward64", "done"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (t, k)
    ra, rb = a.export_state(), b.export_state()
    assert all(np.array_equal(x, y) for x, y in zip(ra, rb))
    assert a.reset_count() == b.reset_count()
    _finish(a); _finish(b)


# ---- 2. a range import against the host build ------------------------------------------------------------------------------------------------
def _import_case(gpu, monkeypatch, level, ev, ev_src, done_actions, first, count, pos, repeat=False):
    run = sr.import_run(level, first, count, pos, done_actions, False, repeat)
    model = run["model"]
    # the imported envs' next levels must be the recipient's own: enough of them reach one (the model alone; tests/test_scenario_host.py too)
    assert int(run["restarted"].sum()) * 4 >= count, (int(run["restarted"].sum()), count)
    d = _donor(gpu, monkeypatch, level, ev_src, done_actions)
    rec, hot, stale = d.export_state()
    d.close()
    events = [("import", {"rec": rec[run["src"]], "hot": hot[run["src"]], "stale": stale[run["src"]]}, first) if e[0] == "import" else e for e in run["events"]]
    env = _make(gpu, monkeypatch, level, ev, sr.RECIPIENT_SEED, done_actions)
    twin = _make(gpu, monkeypatch, level, ev, sr.RECIPIENT_SEED, done_actions)
    got = su.run_device(env, events, "step")
    other = su.run_device(twin, sr.twin_script(events), "step")
    su.assert_equals_model(got, model)
    assert len(got["steps"]["done"]) == model["T"] == run["pre"] + sr.AFTER
    _state_equals("final", env, run["final"])
    _outside_equal_twin(got, other, first, count)
    _finish(twin)
    _finish(env, model["starts"])


CASES2 = [(lv, ev, ev, da, f, c, k % B, False) for lv, ev, da in LAYOUTS for k, (f, c) in enumerate(RANGES)] + \
    [(G, IP1, IP1, False, 64, 64, 1, True), (BOSS, IP0, IP0, False, 64, 64, 2, True),          # donor row 5 in seven envs
     (G, IP1, IP0, False, 1, 190, 3, False), (BOSS, IP0, IP1, False, 1, 190, 0, False)]        # the donor in the other layout
IDS2 = ["%s-%s-pos%d" % (l, r, k % B) for l in LIDS for k, r in enumerate(RIDS)] + \
    ["GoToLocal-inplace1-64+64-row-repeated", "BossLevel-inplace0-64+64-row-repeated", "GoToLocal-classic-to-inplace-1+190", "BossLevel-inplace-to-classic-1+190"]


@pytest.mark.gpu
@pytest.mark.parametrize("level,ev,ev_src,done_actions,first,count,pos,repeat", CASES2, ids=IDS2)
def test_range_import_steps_as_the_host_model(gpu, monkeypatch, level, ev, ev_src, done_actions, first, count, pos, repeat):
    _import_case(gpu, monkeypatch, level, ev, ev_src, done_actions, first, count, pos, repeat)


# ---- 3. hot / stale-only imports --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("level,ev", [(G, IP1), (G, {"BBAI_INPLACE": "1", "BBAI_CPLANE": "0"}), (BOSS, IP0), (G, IP0)],
                         ids=["GoToLocal-inplace1", "GoToLocal-inplace1-cplane0", "BossLevel-inplace0", "GoToLocal-inplace0"])
def test_imports_without_records_move_the_poses_only(gpu, monkeypatch, level, ev):
    """rec = NULL through the library handle (scenario_util.abi_import).  sr.pose_run says why every imported pose is valid for the record it
    meets.  In the in-place layout with a C plane this is the only path that copies the live records out before it rebuilds the C plane rows."""
    run = sr.pose_run(level)
    env = _make(gpu, monkeypatch, level, ev, sr.RECIPIENT_SEED + 2000)
    if ev == IP1:
        assert env.get_option("cplane") == 1
    got = su.run_device(env, run["events"], "step")
    su.assert_equals_model(got, run["model"])
    _state_equals("final", env, run["final"])
    _finish(env, run["model"]["starts"])


# ---- 4. done-action mode -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ev", [IP0, IP1], ids=["inplace0", "inplace1"])
def test_import_in_done_action_mode_clears_last_step_match(gpu, monkeypatch, ev):
    case = sr.done_case()
    model, pre = case["model"], case["pre"]
    matched = np.nonzero(case["is_matched"])[0]
    assert len(matched) >= 1 and bool((case["donor_paid"] > 0).all())          # in the donor itself `done` pays these envs
    d = _make(gpu, monkeypatch, G, ev, sr.DONOR_SEED + 3000, True)
    _steps(d, _dev(gpu, case["donor_acts"]))
    assert np.array_equal((d.save_state().lsm != 0).cpu().numpy().astype(np.uint8), case["donor_lsm"])
    rec, hot, stale = d.export_state()
    d.close()
    src = case["src"]
    events = [("import", {"rec": rec[src], "hot": hot[src], "stale": stale[src]}, sr.DONE_FIRST) if e[0] == "import" else e for e in case["events"]]
    env = _make(gpu, monkeypatch, G, ev, sr.RECIPIENT_SEED + 3000, True)
    got = su.run_device(env, events, "step")
    first_reward = got["steps"]["reward64"][pre][sr.DONE_FIRST + matched]
    assert not first_reward.any(), first_reward          # lastStepMatch is no part of the exported state: `done` fails
    assert bool((got["steps"]["done"][pre][sr.DONE_FIRST:sr.DONE_FIRST + sr.DONE_COUNT] != 0).all())
    su.assert_equals_model(got, model)
    _state_equals("final", env, case["final"])
    _finish(env, model["starts"])


# ---- 5. pixels follow ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tile_size", [8, 16])
def test_pixels_follow_an_import(gpu, monkeypatch, tile_size):
    """An import writes no observation; the next step's does, and its frame must be the whole new view of the imported envs (tile size 8: the
    delta render against the frame the import left behind)."""
    import torch
    first, count = 63, 66
    d = _donor(gpu, monkeypatch, G, IP1)
    rec, hot, stale = d.export_state()
    d.close()
    src = sr.donor_sources(count)
    env = _make(gpu, monkeypatch, G, IP1, sr.RECIPIENT_SEED + 4000, pixel=True, tile_size=tile_size)
    acts = _dev(gpu, su._acts(8, N, 91, 0.0))
    _steps(env, acts[:5])
    before = env.image.clone()
    env.import_state(rec[src], hot[src], stale[src], first=first)
    assert torch.equal(env.image, before)
    changed = 0
    for t in range(5, 8):
        obs, _, _, _ = env.step(acts[t])
        assert obs["image"] is env.pixels
        assert torch.equal(env.pixels, env.render_encoding(env.image, out=torch.zeros_like(env.pixels))), ("step", t)
        if t == 5:
            changed = int((env.image[first:first + count] != before[first:first + count]).reshape(count, -1).any(1).sum())
    assert changed >= count // 2          # (the imported envs do show other views)
    _finish(env)


# ---- 6. token rows -------------------------------------------------------------------------------------------------------------------------------
CASES6 = [(lv, ev, f, c, k % B) for lv in (BOSS, G) for ev in (IP0, IP1) for k, (f, c) in enumerate([(0, 192), (63, 2), (130, 62)])]


@pytest.mark.gpu
@pytest.mark.parametrize("level,ev,first,count,pos", CASES6, ids=["%s-inplace%s-%d+%d" % (lv, ev["BBAI_INPLACE"], f, c) for lv, ev, f, c, _ in CASES6])
def test_token_rows_follow_an_import(gpu, monkeypatch, level, ev, first, count, pos):
    """The registered token rows of the range are the imported missions' right behind the import (no step in between), every other row stays, and
    the steps behind it -- the rollout entry with a token buffer -- keep them to the model's."""
    import torch
    run = sr.import_run(level, first, count, pos)
    model, src = run["model"], run["src"]
    d = _donor(gpu, monkeypatch, level, ev, tokens=True)
    rec, hot, stale = d.export_state()
    donor_instr = d.instr.cpu().numpy()
    d.close()
    su._same("donor token rows", donor_instr, sr.donor(level).tokens())
    events = [("import", {"rec": rec[src], "hot": hot[src], "stale": stale[src]}, first) if e[0] == "import" else e for e in run["events"]]
    env = _make(gpu, monkeypatch, level, ev, sr.RECIPIENT_SEED, tokens=True)
    seen = {}

    def after(kind, index):
        if kind == "import":
            seen["instr"] = env.instr.cpu().numpy()

    k_imp = [e[0] for e in events].index("import")
    head = su.run_device(env, events[:k_imp], "rollout_tokens")
    before = env.instr.cpu().numpy()
    tail = su.run_device(env, events[k_imp:], "rollout_tokens", after=after)
    rng_ = np.arange(first, first + count)
    out = np.setdiff1d(np.arange(N), rng_)
    su._same("imported token rows", seen["instr"][rng_], donor_instr[src])
    su._same("token rows outside the range", seen["instr"][out], before[out])
    assert (seen["instr"][rng_] != before[rng_]).any()
    su._same("token rows behind the import vs the model", seen["instr"], model["imports"][0]["tokens"])
    pre = run["pre"]
    want_head = {"T": pre, "steps": {k: v[:pre] for k, v in model["steps"].items()}, "calls": [], "snaps": [], "bot": {}}
    want_tail = {"T": sr.AFTER, "steps": {k: v[pre:] for k, v in model["steps"].items()}, "calls": [], "snaps": [], "bot": {}, "imports": model["imports"]}
    head["bot"], tail["bot"] = {}, {}
    su.assert_equals_model(head, want_head)
    su.assert_equals_model(tail, want_tail)
    assert tail["steps"]["tokens"][-1] is not None          # (the token rows behind the last step were compared)
    _state_equals("final", env, run["final"])
    _finish(env, model["starts"])


# ---- 7. a fresh expert -----------------------------------------------------------------------------------------------------------------------------
def _expert_recipient(gpu, monkeypatch, case, group=0):
    import torch
    b = _make(gpu, monkeypatch, sr.BOT_LEVEL, IP0, sr.RECIPIENT_SEED + 1000)
    if group:
        b.set_option("bot_group", group)
        try:
            b.bot_actions()
        except Exception as exc:                 # the shipped library carries no k_botg (an experiment build)
            if "built without the lane-group expert" in str(exc):
                b.close()
                return None
            raise
        b.close()
        b = _make(gpu, monkeypatch, sr.BOT_LEVEL, IP0, sr.RECIPIENT_SEED + 1000)
        b.set_option("bot_group", group)
    for t in range(sr.BOT_STEPS):              # the expert on every env: the plans of the envs still in their first episode expect step 10 next
        act = b.bot_actions().clone()
        act[act == b.BOT_GAVE_UP] = b.RESET_ENV
        assert np.array_equal(act.cpu().numpy(), case["expert_acts"][t]), t
        b.step(act)
    return b


@pytest.mark.gpu
def test_an_import_starts_a_fresh_expert(gpu, monkeypatch):
    """BossLevel: recipient and donor have both run 10 steps, so in 33 of the 37 imported pairs (sr.expert_case, counted on the host model;
    at least 8 are required) the row's Hot.step is the 10 that the env's surviving plan would expect -- a plan kept across the import would be
    continued on another level.  The decisions behind the import are the model's with a fresh Bot in the range -- which is also what a handle
    that never consulted the expert decides on the same rows -- and an undisturbed twin's outside it."""
    import torch
    case = sr.expert_case()
    assert int(case["colliding"].sum()) >= 8, int(case["colliding"].sum())
    first, count, src = sr.BOT_FIRST, sr.BOT_COUNT, case["src"]
    d = _make(gpu, monkeypatch, sr.BOT_LEVEL, IP0, sr.DONOR_SEED + 1000)
    _steps(d, _dev(gpu, case["donor_acts"]))
    rec, hot, stale = d.export_state()
    d.close()
    for k in ("rec", "stale"):
        su._same("donor rows " + k, {"rec": rec, "stale": stale}[k][src], case["rows"][k])
    su._same("donor rows hot", hot[src, :15], case["rows"]["hot"][:, :15])
    c = _make(gpu, monkeypatch, sr.BOT_LEVEL, IP0, 6000, n=count)          # never consulted the expert
    c.import_state(rec[src], hot[src], stale[src])
    never = c.bot_actions().cpu().numpy()
    c.close()
    rng_ = np.arange(first, first + count)
    out = np.setdiff1d(np.arange(N), rng_)
    for group in (0, 16):
        b = _expert_recipient(gpu, monkeypatch, case, group)
        if b is None:
            continue                             # (no lane-group expert in this build: the lane-per-env one has been checked)
        twin = _expert_recipient(gpu, monkeypatch, case, group)
        b.import_state(rec[src], hot[src], stale[src], first=first)
        got, got_twin = b.bot_actions().cpu().numpy(), twin.bot_actions().cpu().numpy()
        su._same("decisions of the imported envs vs a fresh Bot (group %d)" % group, got[rng_], case["want"][rng_])
        su._same("decisions of the imported envs vs a handle that never used the expert", got[rng_], never)
        su._same("decisions outside the range vs the twin", got[out], got_twin[out])
        su._same("the twin's decisions vs the model", got_twin, case["want_twin"])
        _finish(b); _finish(twin)


# ---- 8. edges ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ev", [IP0, IP1], ids=["inplace0", "inplace1"])
def test_empty_ranges_and_ranges_outside_the_batch(gpu, monkeypatch, ev):
    import torch
    from babyai_amd.engine import EngineError
    acts = _dev(gpu, su._acts(22, N, 92, 0.0))
    a, b = (_make(gpu, monkeypatch, G, ev, 900, tokens=True) for _ in range(2))
    _steps(a, acts[:10]); _steps(b, acts[:10])
    a.bot_actions(); b.bot_actions()                     # (expert state allocated: the import's memset has something to miss)
    state0, instr0 = a.export_state(), a.instr.clone()
    rows = {"rec": state0[0][:3].copy(), "hot": state0[1][:3].copy(), "stale": state0[2][:3].copy()}
    empty = {k: v[:0] for k, v in rows.items()}
    lib, h = a.lib, a.handle
    P = lambda x: x.ctypes.data
    for first in (0, N):
        su.abi_import(a, empty, first)
        su.abi_import(a, {"rec": None, "hot": empty["hot"], "stale": None}, first)
        r, hh, s = a.export_state(first, 0)
        assert r.shape == (0, a.cfg.rec_bytes) and hh.shape == (0, 16) and s.shape == (0,)
        assert lib.bbai_get_programs(h, first, 0, P(np.zeros(112, np.uint8))) == 0
    assert all(np.array_equal(x, y) for x, y in zip(a.export_state(), state0)) and torch.equal(a.instr, instr0)
    buf = {"rec": np.zeros((4, a.cfg.rec_bytes), np.uint8), "hot": np.zeros((4, 16), np.uint8), "stale": np.zeros(4, np.uint64), "prog": np.zeros((4, 112), np.uint8)}
    for first, count in ((N - 2, 3), (N, 1), (-1, 2), (-1, 0), (0, -1), (N + 1, 0), (5, N)):
        for what, call in (("export", lambda: lib.bbai_export_state(h, first, count, P(buf["rec"]), P(buf["hot"]), P(buf["stale"]))),
                           ("import", lambda: lib.bbai_import_state(h, first, count, P(rows["rec"]), P(rows["hot"]), P(rows["stale"]))),
                           ("programs", lambda: lib.bbai_get_programs(h, first, count, P(buf["prog"])))):
            a.get_option("inplace")                                             # (any successful call in between)
            rc = call()
            assert rc == -1, (what, first, count, rc)                          # BBAI_ERR_ARG, refused before any buffer is touched
            assert b"out of bounds" in lib.bbai_last_error(), (what, first, count)
    with pytest.raises(EngineError, match="out of bounds"):
        a.export_state(N - 1, 2)
    assert all(np.array_equal(x, y) for x, y in zip(a.export_state(), state0)) and torch.equal(a.instr, instr0)
    assert not any(v.any() for v in buf.values())
    assert torch.equal(a.bot_actions(), b.bot_actions())
    for t in range(10, 22):
        a.step(acts[t]); b.step(acts[t])
        for k in ("image", "direction", "reward", "reward64", "done", "instr"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (t, k)
    assert all(np.array_equal(x, y) for x, y in zip(a.export_state(), b.export_state())) and a.reset_count() == b.reset_count()
    _finish(a); _finish(b)
