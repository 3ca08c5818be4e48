"""The full-grid picture's C entry points: declared by include/bbai.h, bound by babyai_amd/engine.py, exported by the built library."""
import ctypes
import os

from test_abi import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bbai_set_grid_atlas", "bbai_render_grid")


def test_header_declares_the_grid_render_entries():
    from babyai_amd import engine
    for name in NAMES:
        assert name in declared_symbols(), name
        assert name in engine.EXPORTED_SYMBOLS, name


def test_library_exports_the_grid_render_entries():
    import __graft_entry__
    __graft_entry__.build()
    import torch  # noqa: F401  (torch's HIP runtime first, as the product loads it)
    lib = ctypes.CDLL(os.path.join(ROOT, "babyai_amd", "libbbai_hip.so"))
    for name in NAMES:
        assert hasattr(lib, name), name


def test_render_grid_rejects_unknown_tile_sizes_without_a_gpu():
    """Argument checks come before any device work: a null handle or a tile size without an atlas format is BBAI_ERR_ARG."""
    import __graft_entry__
    __graft_entry__.build()
    import torch  # noqa: F401
    from babyai_amd import engine
    lib = engine.bind(ctypes.CDLL(os.path.join(ROOT, "babyai_amd", "libbbai_hip.so")))
    assert lib.bbai_render_grid(None, 8, 1, None, 1, None, None) == -1
    assert lib.bbai_set_grid_atlas(None, 12, None, 1, None) == -1
