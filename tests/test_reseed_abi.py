"""bbai_reseed's C entry point and its Python surface, without a GPU: declared by include/bbai.h, bound by babyai_amd/engine.py, exported by
the built library; argument checks before any device work; reseed's refusals on a bare env; the adapters; evaluate_policy's pool switch."""
import ctypes
import os

import numpy as np
import pytest

from test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bbai_reseed"


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    import torch  # noqa: F401  (torch's HIP runtime first, as the product loads it)
    from babyai_amd import engine
    return engine.bind(ctypes.CDLL(os.path.join(ROOT, "babyai_amd", "libbbai_hip.so")))


def test_header_declares_the_entry():
    from babyai_amd import engine
    assert NAME in declared_symbols()
    assert NAME in engine.EXPORTED_SYMBOLS


def test_library_exports_the_entry():
    assert hasattr(_lib(), NAME)


def test_null_handle_calls_are_argument_errors():
    lib = _lib()
    buf = (ctypes.c_uint64 * 4)()
    for count in (0, 1, -1):
        assert lib.bbai_reseed(None, None, None, count, None, None, None) == -1
        assert lib.bbai_reseed(None, None, ctypes.addressof(buf), count, ctypes.addressof(buf), ctypes.addressof(buf), None) == -1


def _bare_env(level="GoToLocal", n=8):
    """A BatchedBabyAIEnv with what reseed's checks read and no handle: they run before any device work."""
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    from babyai_amd.levels import make_cfg
    env = BatchedBabyAIEnv.__new__(BatchedBabyAIEnv)
    env.torch, env.env_id, env.cfg, env.num_envs, env.done_actions, env.handle = torch, "BabyAI-%s-v0" % level, make_cfg(level), n, False, None
    env.device = torch.device("cpu")
    return env


def test_reseed_refuses_before_any_device_work():
    env = _bare_env()
    with pytest.raises(ValueError, match="twice"):
        env.reseed([1, 5, 1], [7, 8, 9])
    with pytest.raises(ValueError, match="twice"):
        env.reseed(np.array([2, 2, 7]), np.array([1, 2, 3], dtype=np.uint64))
    with pytest.raises(ValueError, match="twice"):
        env.reseed([-1, 3, -1, 8, 3], [1, 2, 3, 4, 5])  # (padding may repeat, an env may not)
    k, _ = env._reseed_args([-1, 3, -1, 8, 8 + 4], [1, 2, 3, 4, 5])
    assert k == 5
    with pytest.raises(ValueError, match="seeds"):
        env.reseed([1, 5], [7, 8, 9])                   # two envs, three seeds
    with pytest.raises(ValueError, match="seeds"):
        env.reseed(None, [7, 8, 9])                     # every env (8), three seeds
    with pytest.raises(ValueError, match="seeds"):
        env.reseed([1, 2, 3], np.array([4, 5], dtype=np.uint64))
    with pytest.raises(ValueError, match="negative"):
        env.reseed([1, 5], [7, -8])
    with pytest.raises(ValueError, match="negative"):
        env.reseed([1, 5], np.array([7, -8], dtype=np.int64))
    with pytest.raises(ValueError):
        env.reseed([1], [1 << 64])


def test_reseed_args_convert_seeds():
    import torch
    env = _bare_env()
    k, t = env._reseed_args([3, 0], [5, (1 << 64) - 1])
    assert k == 2 and t.dtype == torch.int64 and t.tolist() == [5, -1]           # (the same 64 bits)
    k, t = env._reseed_args(None, np.arange(8, dtype=np.uint64) + np.uint64(10 ** 9))
    assert k == 8 and t.tolist() == list(range(10 ** 9, 10 ** 9 + 8))
    k, t = env._reseed_args(torch.tensor([1, 2], dtype=torch.int64), torch.tensor([9, 10], dtype=torch.int64))
    assert k == 2 and t.tolist() == [9, 10]
    with pytest.raises(ValueError):
        env._reseed_args([1, 2], torch.tensor([9.0, 10.0]))
    k, t = env._reseed_args([], [])
    assert k == 0 and t.numel() == 0


def test_adapters_pass_reseeds_through():
    from babyai_amd import vec_env

    class Stub(object):
        def reseed(self, ids, seeds):
            import torch
            self.got = (ids, seeds)

            class M(list):
                def snapshot(self):
                    return self
            return {"image": torch.zeros((2, 7, 7, 3), dtype=torch.uint8), "direction": torch.tensor([1, 3], dtype=torch.uint8), "mission": M(["a", "b"])}

    for cls in (vec_env.BatchedParallelEnv, vec_env.BatchedManyEnvs):
        st = Stub()
        v = cls("BabyAI-GoToLocal-v0", 2, engine=st)
        if cls is vec_env.BatchedManyEnvs:
            v.done = [True, True]
        obs = v.reseed([1, -1], [41, 42])
        assert st.got == ([1, -1], [41, 42])
        assert len(obs) == 2 and obs[1]["direction"] == 3 and obs[0]["mission"] == "a"
        if cls is vec_env.BatchedManyEnvs:
            assert v.done == [True, False]               # the reseeded env is live again, the padding entry names none
            v.reseed(None, [1, 2])
            assert v.done == [False, False]


def test_pool_evaluation_refuses_agents():
    from babyai_amd.evaluate import evaluate_policy
    with pytest.raises(ValueError, match="pool"):
        evaluate_policy(None, "BabyAI-GoToLocal-v0", 1, 4, pool=2, agent=object())
    with pytest.raises(ValueError, match="pool"):
        evaluate_policy(None, "BabyAI-GoToLocal-v0", 1, 4, pool=0)
