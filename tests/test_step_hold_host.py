"""The hold action's Python surface without a GPU (include/bbai.h BBAI_ACTION_HOLD, option "step_hold"): step(ids=...) on a bare
BatchedBabyAIEnv over a recording stand-in for the library -- the byte vector the native step is handed, the option set around the call and put
back, the persistent buffer all-HOLD again afterwards, the refusals before any device work, and which actions validation lets through."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 12


class FakeLib(object):
    """bbai_step / bbai_set_option / bbai_get_option as the binding calls them; every call is logged."""

    def __init__(self, step_hold=0, fail=False):
        self.options = {"step_hold": step_hold}
        self.calls = []
        self.fail = fail

    def bbai_set_option(self, handle, name, value):
        self.calls.append(("set", name.decode(), int(value)))
        self.options[name.decode()] = int(value != 0)
        return 0

    def bbai_get_option(self, handle, name, out):
        out._obj.value = self.options[name.decode()]
        return 0

    def bbai_step(self, handle, actions_ptr, *rest):
        got = np.ctypeslib.as_array((ctypes.c_uint8 * N).from_address(actions_ptr)).copy()
        self.calls.append(("step", got, self.options["step_hold"]))
        return -1 if self.fail else 0

    def bbai_last_error(self):
        return b"stand-in failure"


def bare_env(lib, validate_actions=False):
    """What step() reads, and no handle (the pattern of tests/test_reseed_abi.py): a CPU "device", the five output tensors' pointers."""
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    from babyai_amd.levels import make_cfg
    env = BatchedBabyAIEnv.__new__(BatchedBabyAIEnv)
    env.torch, env.env_id, env.cfg, env.num_envs, env.done_actions, env.handle = torch, "BabyAI-GoToLocal-v0", make_cfg("GoToLocal"), N, False, None
    env.device = torch.device("cpu")
    env.lib, env.validate_actions, env.auto_reset = lib, validate_actions, True
    env.full_obs = env.pixel = False
    env.kernel_events, env._hold, env._obs_version, env.tile_size = None, {}, 0, 8
    env.image = torch.zeros((N, 7, 7, 3), dtype=torch.uint8)
    env.direction = torch.zeros((N,), dtype=torch.uint8)
    env.reward = torch.zeros((N,), dtype=torch.float32)
    env.reward64 = torch.zeros((N,), dtype=torch.float64)
    env.done = torch.zeros((N,), dtype=torch.uint8)
    env._out_ptrs = tuple(t.data_ptr() for t in (env.image, env.direction, env.reward, env.reward64, env.done))
    env._stream = lambda: None
    return env


def steps(lib):
    return [c for c in lib.calls if c[0] == "step"]


def sets(lib):
    return [c[1:] for c in lib.calls if c[0] == "set"]


def test_the_constant_is_the_headers():
    from babyai_amd.engine import BatchedBabyAIEnv
    text = open(os.path.join(ROOT, "include", "bbai.h")).read()
    assert "#define BBAI_ACTION_HOLD 8\n" in text and "#define BBAI_ACTION_RESET_ENV 7\n" in text
    assert BatchedBabyAIEnv.HOLD == 8 and BatchedBabyAIEnv.RESET_ENV == 7
    assert '{"step_hold", nullptr, &bbai_env::step_hold, 0, FLAG}' in open(os.path.join(ROOT, "babyai_amd", "csrc", "bbai_engine.hip")).read()


@pytest.mark.parametrize("kind", ["list", "ndarray", "tensor"])
def test_listed_envs_get_their_actions_and_the_rest_hold(kind):
    import torch
    lib = FakeLib()
    env = bare_env(lib)
    ids, acts = [9, 0, 4], [2, 6, 7]
    want = np.full(N, 8, dtype=np.uint8)
    want[ids] = acts
    given = ids if kind == "list" else np.array(ids) if kind == "ndarray" else torch.tensor(ids, dtype=torch.int64)
    _, reward, done, _ = env.step(torch.tensor(acts, dtype=torch.uint8) if kind == "tensor" else acts, ids=given)
    assert reward is env.reward and done is env.done
    (call,) = steps(lib)
    assert np.array_equal(call[1], want)
    assert call[2] == 1                                         # the option was on while the native step was enqueued
    assert sets(lib) == [("step_hold", 1), ("step_hold", 0)] and lib.options["step_hold"] == 0
    assert env._hold_actions[:N].tolist() == [8] * N            # ... and the persistent buffer is all-HOLD again
    buf = env._hold_actions.data_ptr()
    env.step([1], ids=[11])
    assert env._hold_actions.data_ptr() == buf                  # persistent: the same buffer serves every call
    want = np.full(N, 8, dtype=np.uint8)
    want[11] = 1
    assert np.array_equal(steps(lib)[1][1], want)
    assert env._hold_actions[:N].tolist() == [8] * N


def test_an_option_that_is_on_stays_on():
    lib = FakeLib(step_hold=1)
    env = bare_env(lib)
    env.step([3, 3], ids=[1, 2])
    assert sets(lib) == [] and lib.options["step_hold"] == 1 and steps(lib)[0][2] == 1


def test_the_option_is_put_back_when_the_native_call_fails():
    from babyai_amd.engine import EngineError
    lib = FakeLib(fail=True)
    env = bare_env(lib)
    with pytest.raises(EngineError):
        env.step([3, 3], ids=[1, 2])
    assert sets(lib) == [("step_hold", 1), ("step_hold", 0)] and lib.options["step_hold"] == 0
    assert env._hold_actions[:N].tolist() == [8] * N


def test_ids_that_name_no_env_are_skipped_and_may_repeat():
    lib = FakeLib()
    env = bare_env(lib)
    env.step([1, 2, 3, 4], ids=[-1, 5, N, -1])
    want = np.full(N, 8, dtype=np.uint8)
    want[5] = 2
    assert np.array_equal(steps(lib)[0][1], want)
    assert env._hold_actions[:N].tolist() == [8] * N
    env.step([], ids=[])                                        # nobody listed: everybody holds
    assert np.array_equal(steps(lib)[1][1], np.full(N, 8, dtype=np.uint8))


def test_refusals_come_before_any_device_work():
    import torch
    lib = FakeLib()
    env = bare_env(lib)
    with pytest.raises(ValueError, match="twice"):
        env.step([1, 2, 3], ids=[4, 7, 4])
    with pytest.raises(ValueError, match="twice"):
        env.step([1, 2, 3], ids=np.array([-1, 7, 7]))
    with pytest.raises(ValueError, match="need 2 actions"):
        env.step([1, 2, 3], ids=[4, 7])
    with pytest.raises(ValueError, match="need %d actions" % N):
        env.step([1, 2, 3])
    with pytest.raises(ValueError, match="ids"):
        env.step([1, 2], ids=torch.tensor([1, 2], dtype=torch.int32))
    with pytest.raises(TypeError):
        env.step(torch.tensor([1.0, 2.0]), ids=[1, 2])
    assert lib.calls == []


def test_validation_knows_hold_exactly_where_it_means_something():
    import torch
    full8 = [8] + [0] * (N - 1)
    # host data is always checked: 8 is unknown with the option off, known with it on or with ids; 9 and negatives never are
    env = bare_env(FakeLib())
    with pytest.raises(AssertionError, match="unknown action"):
        env.step(full8)
    with pytest.raises(AssertionError, match="unknown action"):
        env.step([9], ids=[3])
    with pytest.raises(AssertionError, match="unknown action"):
        env.step([-1], ids=[3])
    assert env.lib.calls == []
    env.step([8, 7], ids=[3, 4])
    on = bare_env(FakeLib(step_hold=1))
    on.step(full8)
    assert steps(on.lib)[0][1].tolist() == full8
    with pytest.raises(AssertionError, match="unknown action"):
        on.step([9] + [0] * (N - 1))
    # device tensors are checked under validate / validate_actions only
    t8, t9 = torch.tensor(full8, dtype=torch.uint8), torch.tensor([9] + [0] * (N - 1), dtype=torch.uint8)
    env = bare_env(FakeLib())
    env.step(t8)                                                # unchecked: the engine defines the byte
    with pytest.raises(AssertionError, match="unknown action"):
        env.step(t8, validate=True)
    with pytest.raises(AssertionError, match="unknown action"):
        bare_env(FakeLib(), validate_actions=True).step(t8)
    on = bare_env(FakeLib(step_hold=1), validate_actions=True)
    on.step(t8)
    with pytest.raises(AssertionError, match="unknown action"):
        on.step(t9)
    env = bare_env(FakeLib(), validate_actions=True)
    env.step(torch.tensor([8], dtype=torch.uint8), ids=[2])
    with pytest.raises(AssertionError, match="unknown action"):
        env.step(torch.tensor([9], dtype=torch.uint8), ids=[2])
    # a wider integer never wraps into a hold: 264 = 256 + 8 becomes 255
    env = bare_env(FakeLib())
    env.step(torch.tensor([264, 8], dtype=torch.int64), ids=[0, 1])
    assert steps(env.lib)[-1][1][:2].tolist() == [255, 8]


def test_lookahead_refuses_bad_lists_before_any_device_work():
    env = bare_env(FakeLib())
    with pytest.raises(ValueError, match="twice"):
        env.lookahead([0], [1, 2, 3, 4, 5, 6, 1])
    with pytest.raises(ValueError, match="scratch env is one of the listed"):
        env.lookahead([0], [1, 2, 3, 4, 5, 6, 0])
    with pytest.raises(ValueError, match="7 each"):
        env.lookahead([0, 1], [2, 3, 4, 5, 6, 7, 8])
    assert env.lib.calls == []
