"""The replay entries of the C ABI without a GPU: include/bbai_demo_replay.h against babyai_amd/engine.py's ABI_REPLAY table, prototype by
prototype (tests/test_binding_host.py does the same for include/bbai.h and ABI), the built library's exports, and the header as plain C."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bbai_demo_replay.h")


def prototypes():
    """{entry: [kind of every parameter]} of the header; kinds "ptr", "i64", "int", "double"."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(bbai_[a-z_]+)\s*\(([^)]*)\)\s*;", text):
        assert ret.strip() == "int" and name not in out, name
        kinds = []
        for p in params.split(","):
            words = [w for w in p.split() if w != "const"]
            kinds.append("ptr" if "*" in p else {"int64_t": "i64", "uint64_t": "i64", "int": "int", "double": "double"}[words[0]])
        out[name] = kinds
    return out


def test_every_replay_prototype_has_its_table_row():
    from babyai_amd import engine
    protos = prototypes()
    assert list(protos) == ["bbai_demo_replay_feed", "bbai_demo_replay_judge"] == list(engine.ABI_REPLAY)
    assert engine.REPLAY_SYMBOLS == tuple(engine.ABI_REPLAY) and not set(engine.ABI_REPLAY) & set(engine.ABI)
    kind = {ctypes.c_void_p: "ptr", ctypes.c_int64: "i64", ctypes.c_int: "int", ctypes.c_double: "double"}
    for name, params in protos.items():
        restype, argtypes = engine.ABI_REPLAY[name]
        assert restype is ctypes.c_int and [kind[t] for t in argtypes] == params, name


def test_the_library_exports_and_binds_the_replay_entries():
    import __graft_entry__
    __graft_entry__.build()
    import torch  # noqa: F401  (torch's HIP runtime first, as the product loads it)
    from babyai_amd import engine
    lib = engine.bind(ctypes.CDLL(os.path.join(ROOT, "babyai_amd", "libbbai_hip.so")))
    for name, (restype, argtypes) in engine.ABI_REPLAY.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_the_replay_header_is_plain_c():
    subprocess.check_call(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", HEADER])


def test_the_replay_entries_refuse_bad_counts_without_a_device():
    """Argument errors come back before any launch (no GPU is touched): n < 0, no demos, a negative job count; n == 0 is a no-op."""
    import __graft_entry__
    __graft_entry__.build()
    from babyai_amd import engine
    lib = engine.load_library()
    feed_ptrs, judge = [None] * 11, lib.bbai_demo_replay_judge
    assert lib.bbai_demo_replay_feed(-1, None, None, None, None, None, 3, 9, *feed_ptrs) == -1
    assert lib.bbai_demo_replay_feed(4, None, None, None, None, None, 0, 9, *feed_ptrs) == -1
    assert lib.bbai_demo_replay_feed(4, None, None, None, None, None, 3, 9, *feed_ptrs) == -1          # null pointers
    assert b"null" in lib.bbai_last_error()
    assert lib.bbai_demo_replay_feed(0, None, None, None, None, None, 3, 9, *feed_ptrs) == 0
    assert judge(-1, None, None, None, None, None, 3, None, None, None, None, 0, None, None, 0, None, None, None, None) == -1
    assert judge(4, None, None, None, None, None, 3, None, None, None, None, 0, None, None, -1, None, None, None, None) == -1
    assert judge(4, None, None, None, None, None, 3, None, None, None, None, 0, None, None, 0, None, None, None, None) == -1
    assert judge(0, None, None, None, None, None, 3, None, None, None, None, 1, None, None, 5, None, None, None, None) == 0
