"""The Python binding of the C ABI, without a GPU: babyai_amd/engine.py's ABI table against every prototype of include/bbai.h, bind() on the built
library and on one that lacks entries, the seed conversion, the id-list resolution and the listed-twice check."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLDER_LACKS = ("bbai_reseed", "bbai_demo_jobs")


def prototypes():
    """{entry: (kind of the return type, [kind of every parameter])} of include/bbai.h; kinds: "ptr", "i64", "int", "double", "str", "void"."""
    text = open(os.path.join(ROOT, "include", "bbai.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)

    def kind(decl, ret=False):
        decl = " ".join(decl.split())
        if "*" in decl:
            return "str" if ret and re.match(r"const char ?\*$", decl) else "ptr"
        words = [w for w in decl.split() if w != "const"]
        base = words[0]                    # (a parameter's name, if it has one, follows its type)
        return {"int64_t": "i64", "uint64_t": "i64", "int": "int", "double": "double", "void": "void"}[base]

    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(bbai_[a-z_]+)\s*\(([^)]*)\)\s*;", text):
        assert name not in out, name
        params = [] if params.strip() == "void" else params.split(",")
        out[name] = (kind(ret, ret=True), [kind(p) for p in params])
    return out


def table_kind(t):
    if t is None:
        return "void"
    if t is ctypes.c_char_p:
        return "str"               # (as a parameter: a pointer, see below)
    if t is ctypes.c_void_p or t in (ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64)):
        return "ptr"
    return {ctypes.c_int64: "i64", ctypes.c_int: "int", ctypes.c_double: "double"}[t]


def test_every_prototype_has_its_table_row():
    from babyai_amd import engine
    protos = prototypes()
    assert len(protos) == 53
    for name, (ret, params) in protos.items():
        assert name in engine.ABI, name
        restype, argtypes = engine.ABI[name]
        assert table_kind(restype) == ret, name
        got = ["ptr" if table_kind(t) == "str" else table_kind(t) for t in argtypes]
        assert len(got) == len(params), (name, len(got), len(params))
        for i, (g, w) in enumerate(zip(got, params)):
            assert g == w, (name, i, g, w)
    assert sorted(engine.ABI) == sorted(protos)                       # no row without a prototype
    assert list(engine.ABI) == list(protos)                           # ... and in the header's order
    assert isinstance(engine.EXPORTED_SYMBOLS, tuple) and engine.EXPORTED_SYMBOLS == tuple(engine.ABI)


def test_bind_sets_every_symbol_of_the_built_library():
    import __graft_entry__
    __graft_entry__.build()
    import torch  # noqa: F401  (torch's HIP runtime first, as the product loads it)
    from babyai_amd import engine
    raw = ctypes.CDLL(os.path.join(ROOT, "babyai_amd", "libbbai_hip.so"))
    lib = engine.bind(raw)
    assert lib is raw and type(lib) is ctypes.CDLL
    for name, (restype, argtypes) in engine.ABI.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert engine.load_library().bbai_reseed.argtypes is not None


def test_bind_passes_over_what_an_older_library_lacks():
    from babyai_amd import engine

    class Fn(object):
        restype, argtypes = "unset", "unset"

    class Older(object):
        def __init__(self):
            for name in engine.ABI:
                if name not in OLDER_LACKS:
                    setattr(self, name, Fn())

    lib = engine.bind(Older())
    for name, (restype, argtypes) in engine.ABI.items():
        if name in OLDER_LACKS:
            assert not hasattr(lib, name)
        else:
            assert getattr(lib, name).restype is restype and getattr(lib, name).argtypes == argtypes, name


def test_seeds_u64():
    from babyai_amd.engine import seeds_u64
    s = seeds_u64([5, (1 << 64) - 1], "t")
    assert s.dtype == np.uint64 and s.flags.c_contiguous and s.view(np.int64).tolist() == [5, -1]          # (the same 64 bits)
    assert s.tobytes()[8:] == b"\xff" * 8
    a = np.arange(8, dtype=np.uint64) + np.uint64(10 ** 9)
    s = seeds_u64(a, "t")
    assert s.dtype == np.uint64 and np.shares_memory(s, a) and s.tolist() == list(range(10 ** 9, 10 ** 9 + 8))
    assert seeds_u64(np.array([7, 8], dtype=np.int64), "t").tolist() == [7, 8]
    assert seeds_u64((np.int32(3), 4), "t").tolist() == [3, 4]
    e = seeds_u64([], "t")
    assert e.dtype == np.uint64 and e.shape == (0,)
    with pytest.raises(ValueError, match="negative"):
        seeds_u64([7, -8], "t")
    with pytest.raises(ValueError, match="negative"):
        seeds_u64(np.array([7, -8], dtype=np.int64), "t")
    with pytest.raises(ValueError, match="uint64"):
        seeds_u64([1 << 64], "t")


def _bare_env(n=8):
    """A BatchedBabyAIEnv with what the id-list helpers read and no handle, on the CPU device."""
    import torch
    from babyai_amd.engine import BatchedBabyAIEnv
    env = BatchedBabyAIEnv.__new__(BatchedBabyAIEnv)
    env.torch, env.num_envs, env.device, env.handle = torch, n, torch.device("cpu"), None
    return env


def test_id_lists_resolve_on_their_own():
    import torch
    env = _bare_env()
    assert env._ids(None) == (8, None, None)
    k, ptr, t = env._ids([3, 0, 9])
    assert k == 3 and t.dtype == torch.int64 and t.tolist() == [3, 0, 9] and ptr == t.data_ptr() and t.is_contiguous()
    k, ptr, t = env._ids(np.array([[1, 2], [3, 4]], dtype=np.int32))           # (host arrays are flattened)
    assert k == 4 and t.tolist() == [1, 2, 3, 4] and ptr == t.data_ptr()
    mine = torch.tensor([5, 6], dtype=torch.int64)
    k, ptr, t = env._ids(mine)
    assert k == 2 and ptr == mine.data_ptr() and t.data_ptr() == mine.data_ptr()
    k, ptr, t = env._ids([])
    assert k == 0 and t.numel() == 0
    with pytest.raises(ValueError, match="int64"):
        env._ids(torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError, match="int64"):
        env._ids(torch.zeros((2, 2), dtype=torch.int64))
    # two lists resolved in a row: two live tensors, neither knows about the other
    ka, pa, ta = env._ids([1, 2, 3])
    kb, pb, tb = env._ids([4, 5])
    assert (ka, kb) == (3, 2) and pa != pb and pa == ta.data_ptr() and pb == tb.data_ptr()
    assert ta.tolist() == [1, 2, 3] and tb.tolist() == [4, 5]
    assert not hasattr(env, "_grid_ids")


def test_an_env_listed_twice_is_refused_on_the_host():
    import torch
    env = _bare_env()
    for padding in (False, True):
        with pytest.raises(ValueError, match="twice"):
            env._no_env_twice("t", [1, 5, 1], padding=padding)
        with pytest.raises(ValueError, match="twice"):
            env._no_env_twice("t", np.array([-1, 3, -1, 8, 3]), padding=padding)
        env._no_env_twice("t", [1, 5, 2], padding=padding)
        env._no_env_twice("t", None, padding=padding)
        env._no_env_twice("t", torch.tensor([1, 1], dtype=torch.int64), padding=padding)          # a device list is not read back
    env._no_env_twice("t", [-1, 3, -1], padding=True)
    env._no_env_twice("t", [8, 3, 8, 12, 12], padding=True)                   # (ids from num_envs on are padding too)
    with pytest.raises(ValueError, match="twice"):
        env._no_env_twice("t", [-1, 3, -1])
