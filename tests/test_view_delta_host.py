"""The geometry of the delta render at tile sizes 16 and 32 (bbai_viewpx.hpp, k_view_delta), without a GPU: the header's plain-C++ function
that says which view cells a 64-byte piece of a frame is drawn from, compiled with g++ from a wrapper this test writes, against a numpy
derivation from byte offsets alone -- piece p covers bytes [64 p, 64 p + 64), byte b is a colour of pixel b // 3 = (7 ts) y + x, which shows
view cell (x // ts) * 7 + y // ts -- and the bytes the "pieces that touch a changed cell" rule stores against bounds worked out from the
alignment of a cell's runs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "babyai_amd", "csrc")
TS = (16, 32)
PIECE = 64

WRAPPER = """
#include "bbai_viewpx.hpp"
extern "C" unsigned long long piece_cells(int ts, int p) {
    return ts == 16 ? bbai::view_piece_cells<16>(p) : bbai::view_piece_cells<32>(p);
}
extern "C" int pieces_per_frame(int ts) { return ts == 16 ? bbai::ViewFrame<16>::NP : bbai::ViewFrame<32>::NP; }
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("view_delta_host")
    src, so = str(d / "wrapper.cpp"), str(d / "libviewdelta.so")
    with open(src, "w") as f:
        f.write(WRAPPER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", CSRC, "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.piece_cells.restype, lib.piece_cells.argtypes = ctypes.c_ulonglong, [ctypes.c_int, ctypes.c_int]
    lib.pieces_per_frame.restype, lib.pieces_per_frame.argtypes = ctypes.c_int, [ctypes.c_int]
    return lib


def cell_of_byte(ts):
    """int[147 ts^2]: the view cell byte b of a frame shows."""
    p = np.arange(147 * ts * ts) // 3
    y, x = p // (7 * ts), p % (7 * ts)
    return (x // ts) * 7 + y // ts


def piece_masks(ts):
    """bool[pieces, 49] from the byte offsets: does piece p hold a byte of cell c."""
    cob = cell_of_byte(ts).reshape(-1, PIECE)
    m = np.zeros((len(cob), 49), bool)
    m[np.arange(len(cob))[:, None], cob] = True
    return m


@pytest.mark.parametrize("ts", TS)
def test_piece_cells_equal_the_byte_offsets(lib, ts):
    want = piece_masks(ts)
    assert 147 * ts * ts % PIECE == 0 and lib.pieces_per_frame(ts) == len(want) == 147 * ts * ts // PIECE
    assert len(want) == (588 if ts == 16 else 2352)
    bits = 1 << np.arange(49, dtype=np.uint64)
    for p in range(len(want)):
        got = np.uint64(lib.piece_cells(ts, p))
        assert np.array_equal((got & bits) != 0, want[p]), (ts, p, hex(int(got)))
        assert int(got) >> 49 == 0
    # every cell's bytes lie in pieces that name it, and a piece names one or two cells (a 16-byte chunk never crosses a tile row)
    assert want.any(axis=0).all() and set(want.sum(axis=1).tolist()) <= {1, 2}
    if ts == 16:          # 336-byte pixel rows are no multiple of 64: some pieces span two pixel rows
        rows = (np.arange(147 * ts * ts) // (21 * ts)).reshape(-1, PIECE)
        assert (rows.min(axis=1) != rows.max(axis=1)).any()


@pytest.mark.parametrize("ts", TS)
def test_stored_bytes_of_random_masks_within_the_alignment_bounds(lib, ts):
    """A changed cell is ts runs of 3 ts bytes, one per pixel row of its tile row, each starting on a multiple of 16 bytes (21 ts and 3 ts are
    multiples of 16).  Whole 64-byte pieces around a run that starts and ends on 16-byte boundaries add at most 64 - 16 = 48 bytes in front
    of it and 48 behind it -- at 32, where runs of 96 bytes start on multiples of 32, at most 32 at each end -- so
    bytes of the changed cells <= bytes stored <= bytes of the changed cells + 2 * 48 per pixel row of each changed cell."""
    cob = cell_of_byte(ts)
    run = 3 * ts
    starts = np.nonzero(np.diff(np.concatenate([[-1], cob])))[0]               # first byte of every run of one cell
    assert (starts % 16 == 0).all() and run % 16 == 0 and (21 * ts) % 16 == 0
    slack = PIECE - 16
    if ts == 32:
        assert (starts % 32 == 0).all() and run % 32 == 0
        slack = PIECE - 32
    masks = np.array([lib.piece_cells(ts, p) for p in range(lib.pieces_per_frame(ts))], dtype=np.uint64)
    rng = np.random.RandomState(ts)
    patterns = [np.zeros(49, bool), np.ones(49, bool)] + [np.arange(49) == c for c in range(49)] + \
               [rng.random_sample(49) < d for d in (1 / 49, 1 / 8, 1 / 4, 1 / 2) for _ in range(25)]
    for pat in patterns:
        m = np.uint64(sum(1 << c for c in np.nonzero(pat)[0]))
        stored = int(((masks & m) != 0).sum()) * PIECE
        cell_bytes = int(pat.sum()) * run * ts
        assert stored >= cell_bytes, (ts, pat.nonzero())
        assert stored <= cell_bytes + 2 * slack * ts * int(pat.sum()), (ts, pat.nonzero())
        assert stored <= cell_bytes + 2 * 48 * ts * int(pat.sum())
        # ... and the stored pieces are the ones the byte offsets say: exactly those that hold a byte of a changed cell
        assert np.array_equal((masks & m) != 0, pat[cob].reshape(-1, PIECE).any(axis=1))
