"""The engine's options by name (include/bbai.h bbai_set_option / bbai_get_option) and the BBAI_* variables bbai_create reads for them: defaults,
normalisation at set and at create, which names are one-way, and "knobs never change bytes" on handles that went through all of it.  The expected
values below are written out by hand (they are the contract of include/bbai.h, not read back from the library).  One level, 130 envs: two full
64-env blocks and a partial one -- nothing here depends on scale."""
import numpy as np
import pytest

ROOM = "BabyAI-GoToLocal-v0"
N = 130
_open = []


def as_is(v):
    return v


def flag(v):
    return int(v != 0)


def at_least(lo):
    return lambda v: max(lo, v)


def tri(v):
    return -1 if v < 0 else int(v != 0)


# (option, variable read at create or None, default, normalisation of a raw value -- at create and at set alike)
KNOBS = [
    ("render_queue", "BBAI_RENDER_QUEUE", -1, as_is),
    ("render_queue_bpc", None, 0, as_is),
    ("render_queue_blocks", None, 0, as_is),
    ("render_delta_sched", None, 0, as_is),
    ("render_delta_tpb", None, 0, as_is),
    ("render_pace", "BBAI_RENDER_PACE", 0, at_least(0)),
    ("render_group", "BBAI_RENDER_GROUP", 0, as_is),
    ("render_tpb", "BBAI_RENDER_TPB", 0, as_is),
    ("render_delta", "BBAI_RENDER_DELTA", 1, flag),
    ("render_delta_bpc", None, 0, at_least(0)),
    ("grid_render_bpc", None, 0, at_least(0)),
    ("render_delta_from_step", None, -1, tri),
    ("step_prio", "BBAI_STEP_PRIO", 1, as_is),
    ("pregen_group", "BBAI_PREGEN_GROUP", 32, as_is),
    ("pregen_blocks", "BBAI_PREGEN_BLOCKS", 16384, at_least(64)),
    ("pregen_min", "BBAI_PREGEN_MIN", 6144, at_least(0)),
    ("pregen_per_group", "BBAI_PREGEN_PER_GROUP", 12, at_least(1)),
    ("lane_blocks", "BBAI_LANE_BLOCKS", 16384, at_least(1)),         # (GoToLocal has the lane generator; 0 on a handle without it)
    ("consume_fused", "BBAI_CONSUME_FUSED", -1, as_is),
    ("gate_strict", "BBAI_GATE_STRICT", 0, flag),
    ("gate_probe", "BBAI_GATE_PROBE", 1, as_is),
    ("bot_group", "BBAI_BOT_GROUP", 0, as_is),
    ("step_render_split", "BBAI_STEP_RENDER_SPLIT", -1, as_is),
    ("rollout_multi", "BBAI_ROLLOUT_MULTI", 1, as_is),
    ("done_action_enum", None, 0, flag),
]
PIECE_DEFAULT = 64                  # "render_piece_bytes": 64 or 128 only
# readable names that bbai_set_option does not store as they come: what a fresh GoToLocal handle reports (a single room: in-place layout with
# its C plane, refill period 64, the lane generator, one look-ahead stream)
SPECIAL_DEFAULTS = {"pregen_lane": 1, "lookahead_streams": 1}
READ_ONLY_DEFAULTS = {"render_delta_valid": 0, "gate_forced_strict": 0, "gate_fault": 0, "profile_step_ticks": 0, "inplace": 1, "cplane": 1,
                      "lookahead_period": 64, "gate_timeouts": 0, "render_pace_effective": 0}
# variables that choose allocations or the specials at create: cleared so that the read-only values above hold
OTHER_VARS = ["BBAI_INPLACE", "BBAI_VPLANE", "BBAI_CPLANE", "BBAI_LOOKAHEAD", "BBAI_RING_GIB", "BBAI_PREGEN_LANE", "BBAI_LOOKAHEAD_STREAMS"]
SET_VALUES = (-3, 0, 1, 5, 1 << 20)
# per variable, (raw value, what the handle reads back): one that the normalisation changes (or, stored as is, an odd one), one ordinary setting
VAR_VALUES = {
    "BBAI_RENDER_QUEUE": ((-3, -3), (2, 2)), "BBAI_RENDER_PACE": ((-4, 0), (3, 3)), "BBAI_RENDER_GROUP": ((-3, -3), (4, 4)),
    "BBAI_RENDER_TPB": ((-3, -3), (512, 512)), "BBAI_RENDER_DELTA": ((7, 1), (0, 0)), "BBAI_STEP_PRIO": ((-3, -3), (2, 2)),
    "BBAI_PREGEN_GROUP": ((-3, -3), (16, 16)), "BBAI_PREGEN_BLOCKS": ((7, 64), (4096, 4096)), "BBAI_PREGEN_MIN": ((-2, 0), (128, 128)),
    "BBAI_PREGEN_PER_GROUP": ((0, 1), (8, 8)), "BBAI_LANE_BLOCKS": ((-5, 1), (256, 256)), "BBAI_CONSUME_FUSED": ((-3, -3), (1, 1)),
    "BBAI_GATE_STRICT": ((-3, 1), (1, 1)), "BBAI_GATE_PROBE": ((-3, -3), (0, 0)), "BBAI_BOT_GROUP": ((-3, -3), (16, 16)),
    "BBAI_STEP_RENDER_SPLIT": ((-3, -3), (1, 1)), "BBAI_ROLLOUT_MULTI": ((-3, -3), (0, 0)),
}


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    for _, var, _, _ in KNOBS:
        if var:
            monkeypatch.delenv(var, raising=False)
    for var in OTHER_VARS:
        monkeypatch.delenv(var, raising=False)
    yield
    while _open:
        _open.pop().close()


def make(gpu):
    from babyai_amd.engine import BatchedBabyAIEnv
    e = BatchedBabyAIEnv(ROOM, N, device=gpu)
    _open.append(e)
    return e


def close(e):
    _open.remove(e)
    e.close()


def check_defaults(e):
    for name, _, default, _ in KNOBS:
        assert e.get_option(name) == default, name
    assert e.get_option("render_piece_bytes") == PIECE_DEFAULT
    for name, default in list(SPECIAL_DEFAULTS.items()) + list(READ_ONLY_DEFAULTS.items()):
        assert e.get_option(name) == default, name


def set_every_value(e):
    """Every stored knob through SET_VALUES; leaves each at norm(SET_VALUES[-1])."""
    for name, _, _, norm in KNOBS:
        for v in SET_VALUES:
            e.set_option(name, v)
            assert e.get_option(name) == norm(v), (name, v)


def restore_defaults(e):
    for name, _, default, _ in KNOBS:
        e.set_option(name, default)
    e.set_option("render_piece_bytes", PIECE_DEFAULT)
    check_defaults(e)


def test_the_table_names_every_variable():
    assert sorted(VAR_VALUES) == sorted(var for _, var, _, _ in KNOBS if var)
    assert len(KNOBS) == len(set(k[0] for k in KNOBS)) == 25


@pytest.mark.gpu
def test_defaults_at_create(gpu):
    check_defaults(make(gpu))


@pytest.mark.gpu
def test_set_then_get_is_normalised(gpu):
    from babyai_amd.engine import EngineError
    e = make(gpu)
    set_every_value(e)
    for v in (64, 128):
        e.set_option("render_piece_bytes", v)
        assert e.get_option("render_piece_bytes") == v
    for v in SET_VALUES + (32, 256):
        with pytest.raises(EngineError):
            e.set_option("render_piece_bytes", v)
        assert e.get_option("render_piece_bytes") == 128


@pytest.mark.gpu
def test_unknown_and_one_way_names(gpu):
    from babyai_amd.engine import EngineError
    e = make(gpu)
    with pytest.raises(EngineError, match="unknown option 'no_such_knob'"):
        e.set_option("no_such_knob", 1)
    with pytest.raises(EngineError, match="unknown option 'no_such_knob'"):
        e.get_option("no_such_knob")
    with pytest.raises(EngineError):
        e.get_option("gate_fault_inject")              # write only
    for name in READ_ONLY_DEFAULTS:
        with pytest.raises(EngineError):
            e.set_option(name, 1)
    check_defaults(e)                                   # none of it stored anything


@pytest.mark.gpu
def test_variables_at_create(gpu, monkeypatch):
    by_var = {var: name for name, var, _, _ in KNOBS if var}
    for which in (0, 1):
        for var, values in VAR_VALUES.items():
            monkeypatch.setenv(var, str(values[which][0]))
        e = make(gpu)
        for var, values in VAR_VALUES.items():
            assert e.get_option(by_var[var]) == values[which][1], (var, values[which])
        for name, var, default, _ in KNOBS:
            if not var:
                assert e.get_option(name) == default, name
        close(e)
    for var in VAR_VALUES:
        monkeypatch.delenv(var)
    check_defaults(make(gpu))


@pytest.mark.gpu
def test_knobs_never_change_bytes(gpu, monkeypatch):
    """A handle whose knobs went through every value, one created under the variables' settings and an untouched one: back at the defaults and
    with the same seeds they step the same bytes."""
    import torch
    a = make(gpu)
    set_every_value(a)
    a.set_option("render_piece_bytes", 128)
    for var, values in VAR_VALUES.items():
        monkeypatch.setenv(var, str(values[1][0]))
    b = make(gpu)
    for var in VAR_VALUES:
        monkeypatch.delenv(var)
    c = make(gpu)
    envs = (a, b, c)
    for e in envs[:2]:
        restore_defaults(e)
    for e in envs:
        e.seed(1000)
        e.reset()
    assert torch.equal(a.image, c.image) and torch.equal(b.image, c.image)
    rng = np.random.RandomState(5)
    for t in range(20):
        act = torch.as_tensor(rng.randint(0, 7, size=N).astype(np.uint8), device=gpu)
        for e in envs:
            e.step(act)
        for e in envs[:2]:
            assert torch.equal(e.image, c.image), t
            assert torch.equal(e.reward64, c.reward64), t
            assert torch.equal(e.done, c.done), t
    assert all(e.gate_timeouts() == 0 for e in envs)
