"""Partial-view pixels at view sizes 3, 5, 7, 9, 11 and tile sizes 8, 16, 32 on the host: the C ABI of the two entries
(include/bbai_view_pixels.h against engine.ABI_VIEW_PIXELS), the kernel's plain-C++ index arithmetic and launch shape
(babyai_amd/csrc/bbai_viewpxn.hpp, compiled here with g++) against a frame written from the picture's geometry alone
(view_pixels_util), and that reference against the oracle's get_obs_render with agent_view_size = V -- which is what ties the GPU
tests' reference (tests/test_gpu_view_pixels.py) to the oracle.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import large_outputs_util as lou
import view_pixels_util as vpu
from oracle import levels as olevels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bbai_set_view_pixels_atlas", "bbai_render_view_pixels")
HEADER = os.path.join(ROOT, "include", "bbai_view_pixels.h")
COMBOS = [(V, ts) for V in vpu.VIEW_SIZES for ts in vpu.TILE_SIZES]
ACTIONS = (0, 1, 2, 2, 2, 2, 3, 3, 5, 5, 4, 6)      # biased towards forward / pickup / toggle

_SRC = r"""
#include "bbai_viewpxn.hpp"
using namespace bbai;
template <int V, int TS> static void geometry(int* g) {
    using F = ViewPxN<V, TS>;
    const int v[10] = {F::CELLS, F::AGENT_CELL, F::ENC_BYTES, F::BYTES, F::F16, F::P, F::PPC, F::TILE_BYTES, F::MAX_ENVS, F::LDS ? 1 : 0};
    for (int i = 0; i < 10; ++i) g[i] = v[i];
}
template <int V, int TS> static void pieces(uint32_t* cell, uint32_t* off) {
    using F = ViewPxN<V, TS>;
    for (uint32_t j = 0; j < (uint32_t)F::F16; ++j)
        for (uint32_t h = 0; h < (uint32_t)F::PPC; ++h) {
            const ViewPxPiece p = viewpxn_piece<V, TS>(j, h);
            cell[j * F::PPC + h] = p.cell; off[j * F::PPC + h] = p.off;
        }
}
#define EACH_TS(V, f, ...) (ts == 8 ? f<V, 8>(__VA_ARGS__) : ts == 16 ? f<V, 16>(__VA_ARGS__) : f<V, 32>(__VA_ARGS__))
#define EACH(f, ...) (v == 3 ? EACH_TS(3, f, __VA_ARGS__) : v == 5 ? EACH_TS(5, f, __VA_ARGS__) : v == 7 ? EACH_TS(7, f, __VA_ARGS__) : \
                      v == 9 ? EACH_TS(9, f, __VA_ARGS__) : EACH_TS(11, f, __VA_ARGS__))
extern "C" void vp_geometry(int v, int ts, int* g) { EACH(geometry, g); }
extern "C" void vp_pieces(int v, int ts, uint32_t* cell, uint32_t* off) { EACH(pieces, cell, off); }
extern "C" void vp_items(int v, int ts, int64_t count, int64_t blocks, int64_t* out) {
    const ViewPxItems it = viewpxn_items(v, ts, count, blocks);
    out[0] = it.envs_per_item; out[1] = it.slices; out[2] = it.items;
}
extern "C" int vp_ok(int v, int ts) { return (viewpxn_view_ok(v) ? 1 : 0) | (viewpxn_tile_ok(ts) ? 2 : 0); }
extern "C" void vp_constants(int* c) { c[0] = VIEWPXN_BLOCK; c[1] = VIEWPXN_ITEM_BYTES; c[2] = VIEWPXN_SLICE_MIN; }
"""


@pytest.fixture(scope="module")
def arith(tmp_path_factory):
    d = tmp_path_factory.mktemp("view_pixels")
    src, so = str(d / "view_pixels.cpp"), str(d / "libview_pixels.so")
    with open(src, "w") as f:
        f.write(_SRC)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas",
                           "-I" + os.path.join(ROOT, "babyai_amd", "csrc"), "-o", so, src])
    L = ctypes.CDLL(so)
    P, I, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    L.vp_geometry.argtypes = [I, I, P]
    L.vp_pieces.argtypes = [I, I, P, P]
    L.vp_items.argtypes = [I, I, I64, I64, P]
    L.vp_ok.argtypes = [I, I]
    L.vp_constants.argtypes = [P]
    for f in (L.vp_geometry, L.vp_pieces, L.vp_items, L.vp_constants):
        f.restype = None
    return L


def geometry(L, V, ts):
    g = np.zeros(10, np.int32)
    L.vp_geometry(V, ts, g.ctypes.data)
    return dict(zip(("cells", "agent", "enc", "bytes", "f16", "p", "ppc", "tile_bytes", "max_envs", "lds"), (int(x) for x in g)))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def prototypes():
    """{entry: [kind of every parameter]} of include/bbai_view_pixels.h; kinds "ptr", "i64", "int"."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(bbai_[a-z_]+)\s*\(([^)]*)\)\s*;", text):
        assert ret.strip() == "int" and name not in out, name
        kinds = []
        for p in params.split(","):
            words = [w for w in p.split() if w != "const"]
            kinds.append("ptr" if "*" in p else {"int64_t": "i64", "int": "int"}[words[0]])
        out[name] = kinds
    return out


def test_every_prototype_has_its_table_row():
    from babyai_amd import engine
    protos = prototypes()
    assert list(protos) == list(NAMES) == list(engine.ABI_VIEW_PIXELS)
    assert engine.VIEW_PIXELS_SYMBOLS == tuple(engine.ABI_VIEW_PIXELS)
    assert not set(engine.ABI_VIEW_PIXELS) & (set(engine.ABI) | set(engine.ABI_REPLAY) | set(engine.ABI_VIEW))
    kind = {ctypes.c_void_p: "ptr", ctypes.c_int64: "i64", ctypes.c_int: "int"}
    for name, params in protos.items():
        restype, argtypes = engine.ABI_VIEW_PIXELS[name]
        assert restype is ctypes.c_int and [kind[t] for t in argtypes] == params, name
    # the atlas entry takes what bbai_set_view_atlas takes; the render entry bbai_render_view's arguments behind a view size
    assert engine.ABI_VIEW_PIXELS["bbai_set_view_pixels_atlas"] == engine.ABI["bbai_set_view_atlas"]
    rv = engine.ABI["bbai_render_view"][1]
    assert engine.ABI_VIEW_PIXELS["bbai_render_view_pixels"][1] == rv[:1] + [ctypes.c_int] + rv[1:]
    subprocess.check_call(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Wextra", "-pedantic", HEADER])
    text = open(HEADER).read()
    for word in ("RGBImgPartialObsWrapper", "ViewSizeWrapper", "get_obs_render", "BBAI_ERR_ARG", "BBAI_ERR_STATE"):
        assert word in text, word


def test_library_exports_the_entries_and_refuses_a_null_handle():
    from babyai_amd import engine
    import __graft_entry__
    __graft_entry__.build()
    import torch  # noqa: F401  (torch's HIP runtime first, as the product loads it)
    lib = engine.bind(ctypes.CDLL(os.path.join(ROOT, "babyai_amd", "libbbai_hip.so")))
    for name in NAMES:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == engine.ABI_VIEW_PIXELS[name][1]
    assert lib.bbai_set_view_pixels_atlas(None, 8, None, 58, None) == -1                          # BBAI_ERR_ARG: null handle
    assert lib.bbai_render_view_pixels(None, 9, 16, None, 1, None, 1, None, None) == -1
    assert b"null handle" in lib.bbai_last_error()


def test_bind_passes_over_a_library_without_the_entries():
    from babyai_amd import engine

    class Old(object):
        pass
    assert engine.bind(Old()) is not None


def test_python_argument_checks_need_no_device():
    """check_view_size / check_tile_size are what render_view and render_encoding ask before any device work."""
    from babyai_amd import engine
    import inspect
    for v in (4, 13, 0, "9", 9.0, True):
        with pytest.raises(ValueError):
            engine.check_view_size(v)
    for ts in (12, 64, 0, 8.5):
        with pytest.raises(ValueError):
            engine.check_tile_size(ts)
    for meth in (engine.BatchedBabyAIEnv.render_view, engine.BatchedBabyAIEnv.render_encoding):
        p = inspect.signature(meth).parameters
        assert "view_size" in p and p["view_size"].default is None, meth
    assert inspect.signature(engine.BatchedBabyAIEnv.render_view).parameters["tile_size"].default is None


# ---- the index arithmetic -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ts", COMBOS)
def test_geometry(arith, V, ts):
    g = geometry(arith, V, ts)
    assert g["cells"] == V * V and g["agent"] == vpu.agent_cell(V) and g["enc"] == 3 * V * V
    assert g["bytes"] == vpu.frame_bytes(V, ts) and g["bytes"] % 64 == 0 and g["f16"] * 16 == g["bytes"]
    assert g["p"] * g["ppc"] == 16 and g["p"] == (8 if ts == 8 else 16)
    assert g["tile_bytes"] == 3 * ts * ts and g["lds"] == (1 if ts <= 16 else 0)
    assert g["max_envs"] * V * V <= 1024 < (g["max_envs"] + 1) * V * V
    assert arith.vp_ok(V, ts) == 3
    assert {V: vpu.agent_cell(V) for V in vpu.VIEW_SIZES} == {3: 5, 5: 14, 7: 27, 9: 44, 11: 65}
    assert vpu.frame_bytes(3, 8) == 1728 and vpu.frame_bytes(11, 32) == 371712


def test_sizes_outside_the_sets(arith):
    for v in (0, 1, 2, 4, 6, 8, 10, 12, 13, -3):
        assert arith.vp_ok(v, 8) == 2, v
    for ts in (0, 4, 12, 24, 64, -8):
        assert arith.vp_ok(7, ts) == 1, ts


@pytest.mark.parametrize("V,ts", COMBOS)
def test_a_frame_assembled_chunk_by_chunk_is_the_reference_frame(arith, V, ts):
    """Every 16-byte chunk of a frame, built from the pieces viewpxn_piece names (the cell's tile id from random ids, P bytes of that
    tile from the piece's offset), against the same 16 bytes of the frame the geometry gives."""
    g = geometry(arith, V, ts)
    n = g["f16"] * g["ppc"]
    cell, off = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    arith.vp_pieces(V, ts, cell.ctypes.data, off.ctypes.data)
    assert int(cell.max()) < V * V and int(off.max()) + g["p"] <= g["tile_bytes"] and (off % g["p"] == 0).all()
    assert set(cell.tolist()) == set(range(V * V))
    tiles, _ = vpu.atlas(ts)
    flat = tiles.reshape(len(tiles), -1)
    rng = np.random.RandomState(100 * V + ts)
    for trial in range(3):
        ids = rng.randint(0, len(tiles), size=(1, V * V)).astype(np.uint8)
        want = vpu.frames_of_ids(ids, V, ts).reshape(g["f16"], 16)
        got = flat[ids[0][cell][:, None], off[:, None].astype(np.int64) + np.arange(g["p"])[None, :]].reshape(g["f16"], 16)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (V, ts, trial, bad[:8].tolist())


def test_tile_size_8_chunks_straddle_tiles_and_pixel_rows(arith):
    """What makes tile size 8 different: at every view size some chunk's two pieces come from two tiles, and some from two pixel rows."""
    for V in vpu.VIEW_SIZES:
        g = geometry(arith, V, 8)
        n = g["f16"] * 2
        cell, off = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        arith.vp_pieces(V, 8, cell.ctypes.data, off.ctypes.data)
        c, o = cell.reshape(-1, 2), off.reshape(-1, 2)
        assert (c[:, 0] != c[:, 1]).any(), V
        assert ((c[:, 0] // V == V - 1) & (c[:, 1] // V == 0)).any(), V          # last column of one pixel row, first of the next


@pytest.mark.parametrize("V,ts", COMBOS)
def test_launch_shape_is_the_headers(arith, V, ts):
    """engine.view_pixels_items (what the GPU tests and the bench size their cases with) = viewpxn_items (what the launch uses); an item
    never holds more envs than the block has lanes for, nor more than VIEWPXN_ITEM_BYTES of frames; slices cover a frame."""
    from babyai_amd import engine
    c = np.zeros(3, np.int32)
    arith.vp_constants(c.ctypes.data)
    assert tuple(int(x) for x in c) == (engine.VIEW_PIXELS_BLOCK, engine.VIEW_PIXELS_ITEM_BYTES, engine.VIEW_PIXELS_SLICE_MIN)
    g = geometry(arith, V, ts)
    out = np.zeros(3, np.int64)
    for cus in (1, 8, 256, 304):
        blocks = cus * engine.VIEW_PIXELS_BLOCKS_PER_CU
        # (... (1 << 22) + 3 and the frame count that crosses 4 GiB at this size: the cases of tests/test_gpu_large_outputs.py)
        for count in (1, 2, 3, 7, 100, blocks - 1, blocks, blocks + 1, 3 * blocks + 1, 20000, 1 << 20, (1 << 22) + 3, lou.count_for(g["bytes"]), 1 << 33):
            arith.vp_items(V, ts, count, blocks, out.ctypes.data)
            epi, slices, items, nb = engine.view_pixels_items(V, ts, count, cus)
            assert (epi, slices, items) == tuple(int(x) for x in out), (V, ts, cus, count)
            assert nb == max(1, min(items, blocks))
            assert 1 <= epi <= g["max_envs"] and slices >= 1 and (epi == 1 or slices == 1)
            assert epi * g["bytes"] <= engine.VIEW_PIXELS_ITEM_BYTES or epi == 1
            assert slices <= g["f16"]
            assert items == (count * slices if slices > 1 else -(-count // epi))
    # the full-size table: items of 64 - 150 KB
    epi, slices, _, _ = engine.view_pixels_items(V, ts, 1 << 20, 256)
    assert 64000 <= epi * g["bytes"] // slices <= 150528, (V, ts, epi, slices)
    assert (slices > 1) == (V >= 9 and ts == 32)


# ---- the reference against the oracle -----------------------------------------------------------------------------------------------
def oracle_env(name, seed, V):
    e = olevels.make_env(name)
    e.agent_view_size = V
    e.seed(seed)
    return e


@pytest.mark.parametrize("name", ["GoToLocal", "BossLevel", "OpenRedDoor", "PutNextS5N2Carrying"])
def test_reference_frames_are_get_obs_render(name):
    """view_pixels_util.frames of the oracle's V x V encoding = the oracle's get_obs_render of it, at every view size but 7 and every tile
    size, along random steps across resets.  (Needs nothing of the feature: it pins the GPU tests' reference.)"""
    steps = 36
    for V in (3, 5, 9, 11):
        ref = oracle_env(name, 40 + V, V)
        rng = np.random.RandomState(V)
        obs = ref.reset()
        encs, want = [], {ts: [] for ts in vpu.TILE_SIZES}
        for t in range(steps + 1):
            assert obs["image"].shape == (V, V, 3)
            encs.append(obs["image"].copy())
            for ts in vpu.TILE_SIZES:
                want[ts].append(ref.get_obs_render(obs["image"], tile_size=ts))
            obs, _, done, _ = ref.step(int(ACTIONS[rng.randint(0, len(ACTIONS))]))
            if done:
                obs = ref.reset()
        enc = np.stack(encs).astype(np.uint8)
        for ts in vpu.TILE_SIZES:
            got = vpu.frames(enc, ts)
            w = np.stack(want[ts])
            assert got.shape == w.shape == (steps + 1, V * ts, V * ts, 3)
            bad = np.nonzero((got != w).reshape(len(w), -1).any(axis=1))[0]
            assert len(bad) == 0, (name, V, ts, bad[:4].tolist())


def test_reference_at_7_is_render_utils():
    import render_util
    enc = render_util.synthetic_encodings(40, 3)
    assert np.array_equal(vpu.tile_ids(enc, 8), render_util.tile_ids(enc))
    assert np.array_equal(vpu.frames(enc, 8), render_util.frames(render_util.tile_ids(enc)))
    assert np.array_equal(vpu.synthetic_encodings(40, 7, 3), enc)
