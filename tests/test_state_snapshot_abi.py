"""Device snapshots' C entry points and their Python surface, without a GPU: declared by include/bbai.h, bound by babyai_amd/engine.py,
exported by the built library; argument checks before any device work; EnvSnapshot's row operations on CPU tensors; load_state's refusals."""
import ctypes
import os

import numpy as np
import pytest

from test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bbai_save_state", "bbai_load_state")


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    import torch  # noqa: F401  (torch's HIP runtime first, as the product loads it)
    from babyai_amd import engine
    return engine.bind(ctypes.CDLL(os.path.join(ROOT, "babyai_amd", "libbbai_hip.so")))


def test_header_declares_the_snapshot_entries():
    from babyai_amd import engine
    for name in NAMES:
        assert name in declared_symbols(), name
        assert name in engine.EXPORTED_SYMBOLS, name


def test_library_exports_the_snapshot_entries():
    lib = _lib()
    for name in NAMES:
        assert hasattr(lib, name), name


def test_null_handle_calls_are_argument_errors():
    lib = _lib()
    for count in (0, 1, -1):
        assert lib.bbai_save_state(None, None, count, None, None, None, None, None) == -1
        assert lib.bbai_load_state(None, None, None, count, 1, None, None, None, None, None, None, None) == -1


def _snap(level="GoToLocal", rows=5, done_actions=False, rec_bytes=None):
    import torch
    from babyai_amd.engine import EnvSnapshot
    from babyai_amd.levels import make_cfg
    rb = make_cfg(level).rec_bytes if rec_bytes is None else rec_bytes
    g = torch.Generator().manual_seed(rows)
    return EnvSnapshot(torch.randint(0, 256, (rows, rb), dtype=torch.uint8, generator=g), torch.randint(0, 256, (rows, 16), dtype=torch.uint8, generator=g),
                       torch.arange(rows, dtype=torch.int64) * 3 - 4, torch.arange(rows, dtype=torch.uint8), "BabyAI-%s-v0" % level, rb, done_actions)


def test_snapshot_rows_on_cpu_tensors():
    import torch
    from babyai_amd.engine import EnvSnapshot
    a, b = _snap(rows=5), _snap(rows=3)
    assert len(a) == 5 and len(b) == 3 and a.env_id == "GoToLocal"
    s = a.select([4, 0, 4])
    assert len(s) == 3 and (s.env_id, s.rec_bytes, s.done_actions) == (a.env_id, a.rec_bytes, a.done_actions)
    for k in ("rec", "hot", "stale", "lsm"):
        assert torch.equal(getattr(s, k), getattr(a, k)[[4, 0, 4]]), k
        assert getattr(s, k).is_contiguous()
    t = a.select(torch.tensor([1, 2], dtype=torch.int64))
    assert torch.equal(t.rec, a.rec[1:3])
    c = EnvSnapshot.cat([a, b, s])
    assert len(c) == 11
    for k in ("rec", "hot", "stale", "lsm"):
        assert torch.equal(getattr(c, k), torch.cat([getattr(a, k), getattr(b, k), getattr(s, k)])), k
    d = c.to("cpu")
    assert len(d) == 11 and torch.equal(d.rec, c.rec) and d.device.type == "cpu"
    assert len(a.select([])) == 0
    with pytest.raises(ValueError):
        EnvSnapshot.cat([a, _snap("BossLevel")])
    with pytest.raises(ValueError):
        EnvSnapshot.cat([a, _snap(done_actions=True)])
    with pytest.raises(ValueError):
        EnvSnapshot.cat([])
    with pytest.raises(ValueError):
        EnvSnapshot(a.rec, a.hot[:2], a.stale, a.lsm, a.env_id, a.rec_bytes, False)


def _bare_env(level="GoToLocal", n=8, done_actions=False):
    """A BatchedBabyAIEnv with what load_state's checks read and no handle: they run before any device work."""
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    from babyai_amd.levels import make_cfg
    env = BatchedBabyAIEnv.__new__(BatchedBabyAIEnv)
    env.torch, env.env_id, env.cfg, env.num_envs, env.done_actions, env.handle = torch, "BabyAI-%s-v0" % level, make_cfg(level), n, done_actions, None
    return env


def test_load_state_refuses_foreign_snapshots_and_duplicate_ids():
    env = _bare_env()
    with pytest.raises(ValueError, match="level"):
        env.load_state(_snap("BossLevel", rows=8))
    with pytest.raises(ValueError, match="records"):
        env.load_state(_snap(rows=8, rec_bytes=env.cfg.rec_bytes + 16))
    with pytest.raises(ValueError, match="done_actions"):
        env.load_state(_snap(rows=8, done_actions=True))
    with pytest.raises(ValueError, match="done_actions"):
        _bare_env(done_actions=True).load_state(_snap(rows=8))
    with pytest.raises(ValueError, match="twice"):
        env.load_state(_snap(rows=3), ids=[1, 5, 1])
    with pytest.raises(ValueError, match="twice"):
        env.load_state(_snap(rows=3), ids=np.array([2, 2, 7]), rows=[0, 1, 2])
    with pytest.raises(ValueError):
        env.load_state(_snap(rows=3), ids=[1, 5])              # three rows for two envs
    with pytest.raises(ValueError):
        env.load_state(_snap(rows=3))                          # every env, from three rows
    with pytest.raises(TypeError):
        env.load_state((1, 2, 3))


def test_adapters_pass_snapshots_through():
    from babyai_amd import vec_env

    class Stub(object):
        def save_state(self, ids=None):
            return ("snap", ids)

        def load_state(self, snap, ids=None, rows=None):
            import torch
            self.got = (snap, ids, rows)

            class M(list):
                def snapshot(self):
                    return self
            return {"image": torch.zeros((2, 7, 7, 3), dtype=torch.uint8), "direction": torch.tensor([1, 3], dtype=torch.uint8), "mission": M(["a", "b"])}

    for cls in (vec_env.BatchedParallelEnv, vec_env.BatchedManyEnvs):
        st = Stub()
        v = cls("BabyAI-GoToLocal-v0", 2, engine=st)
        assert v.save_state([1]) == ("snap", [1])
        obs = v.load_state("s", ids=[0], rows=[1])
        assert st.got == ("s", [0], [1])
        assert len(obs) == 2 and obs[1]["direction"] == 3 and obs[0]["mission"] == "a"
