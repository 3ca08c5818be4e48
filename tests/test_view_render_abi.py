"""The partial-view render's C entry points and its Python surface, without a GPU: declared by include/bbai.h, bound by
babyai_amd/engine.py, exported by the built library; argument checks before any device work; the adapters' observation space."""
import ctypes
import os

import pytest

from test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bbai_set_view_atlas", "bbai_render_view")


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    import torch  # noqa: F401  (torch's HIP runtime first, as the product loads it)
    from babyai_amd import engine
    return engine.bind(ctypes.CDLL(os.path.join(ROOT, "babyai_amd", "libbbai_hip.so")))


def test_header_declares_the_view_render_entries():
    from babyai_amd import engine
    for name in NAMES:
        assert name in declared_symbols(), name
        assert name in engine.EXPORTED_SYMBOLS, name


def test_library_exports_the_view_render_entries():
    lib = _lib()
    for name in NAMES:
        assert hasattr(lib, name), name


def test_null_handle_calls_are_argument_errors():
    lib = _lib()
    for ts in (16, 32, 8, 12):
        assert lib.bbai_set_view_atlas(None, ts, None, 1, None) == -1
        assert lib.bbai_render_view(None, ts, None, 1, None, 1, None, None) == -1


def test_product_loads_the_atlases_only():
    import __graft_entry__
    __graft_entry__.build()
    from babyai_amd import engine
    for ts in (8, 16, 32):
        assert os.path.isfile(engine.VIEW_ATLAS_PATH % ts), ts
    assert engine.VIEW_ATLAS_PATH % 8 == engine.ATLAS_PATH


def test_unknown_partial_view_tile_size_raises_without_a_gpu():
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
                make(pixel=True, tile_size=ts)


@pytest.mark.parametrize("ts", [8, 16, 32])
def test_observation_space_is_the_returned_shape(ts):
    from babyai_amd import vec_env

    class Stub(object):
        pass
    for cls in (vec_env.BatchedParallelEnv, vec_env.BatchedManyEnvs):
        v = cls("BabyAI-GoToLocal-v0", 2, pixel=True, engine=Stub(), tile_size=ts)
        assert v.observation_space["image"].shape == (7 * ts, 7 * ts, 3)
        assert v[0].observation_space["image"].shape == (7 * ts, 7 * ts, 3)
    assert vec_env.BatchedParallelEnv("BabyAI-GoToLocal-v0", 2, pixel=False, engine=Stub()).observation_space["image"].shape == (7, 7, 3)
