"""The delta render's piece rule on the host (babyai_amd/csrc/bbai_render.hpp, store_dirty_pieces; option "render_piece_bytes", default
64): a 64-byte piece of an env's image is stored iff a cell it draws from changed its atlas tile id.  Checked against the reference's own
frames (the golden pixel traces) laid out back to back as the device buffer holds them: storing only the marked pieces over the previous
frame gives the new frame -- 64 divides 9408, so every piece lies inside one env and the rule needs no env pairs; the traces cross resets."""
import glob
import os

import numpy as np
import pytest

from hostsim_util import lib

PIX_BYTES, PIECE = 9408, 64
GOLDEN = [p for p in sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))]


def cell_of_byte():
    """byte of an env's 56x56x3 image -> the cell (view x * 7 + view y) its tile comes from (k_render's render_chunk)."""
    b = np.arange(PIX_BYTES)
    py, cx = b // 168, (b % 168) // 24
    return cx * 7 + (py >> 3)


def piece_table():
    """[147, 49] bool: the cells each 64-byte piece of an env draws from (init_piece_cells)."""
    cob = cell_of_byte().reshape(PIX_BYTES // PIECE, PIECE)
    t = np.zeros((PIX_BYTES // PIECE, 49), bool)
    for p in range(len(t)):
        t[p, np.unique(cob[p])] = True
    return t


def tile_ids(frames):
    """uint8[N, 56, 56, 3] -> int[N, 49]: one id per distinct 8x8 tile content (what the atlas id stands for)."""
    t = frames.reshape(len(frames), 7, 8, 7, 8, 3).transpose(0, 3, 1, 2, 4, 5).reshape(len(frames), 49, 192)
    _, ids = np.unique(t.reshape(-1, 192), axis=0, return_inverse=True)
    return ids.reshape(len(frames), 49)


def test_piece_table():
    t = piece_table()
    assert PIX_BYTES % PIECE == 0 and t.shape == (147, 49)
    assert t.any(axis=1).all() and t.any(axis=0).all()         # every piece draws on a cell, every cell is drawn by a piece
    cob = cell_of_byte()
    for p in range(len(t)):                                    # the marked cells are exactly the cells of the piece's bytes
        assert set(np.nonzero(t[p])[0].tolist()) == set(cob[p * PIECE:(p + 1) * PIECE].tolist())


def test_piece_table_is_the_headers():
    """The numpy table above against line_cells of bbai_render.hpp, called as init_piece_cells calls it: all 147 pieces of an env."""
    L = lib()
    t = piece_table()
    for p in range(len(t)):
        assert L.hs_line_cells(p * PIECE, p * PIECE + PIECE) == sum(1 << int(c) for c in np.nonzero(t[p])[0]), p


@pytest.mark.parametrize("path", [p for p in GOLDEN if os.path.basename(p) in ("BossLevel.npz", "GoToLocal.npz")])      # (the traces with pixel frames)
def test_piece_rule_against_brute_force(path):
    with np.load(path, allow_pickle=False) as f:
        pix = f["pixels"]
    assert pix.shape[1] > 0
    T, N = pix.shape[:2]
    table = piece_table()
    ids = tile_ids(pix.reshape(T * N, 56, 56, 3)).reshape(T, N, 49)
    npe = PIX_BYTES // PIECE
    stored_total = line_total = changed_total = 0
    for t in range(1, T):
        prev, cur = pix[t - 1].reshape(-1), pix[t].reshape(-1)
        dirty = ids[t] != ids[t - 1]                                       # [N, 49]
        marked = (dirty.astype(np.uint8) @ table.T.astype(np.uint8) > 0).reshape(-1)          # [N * 147]: piece q of the flat buffer
        diff = (prev != cur).reshape(N * npe, PIECE).any(axis=1)
        assert not (diff & ~marked).any(), t                               # every changed piece is stored
        out = prev.reshape(N * npe, PIECE).copy()
        out[marked] = cur.reshape(N * npe, PIECE)[marked]
        assert np.array_equal(out.reshape(-1), cur), t
        stored_total += int(marked.sum()) * PIECE
        changed_total += int(diff.sum()) * PIECE
        lines = np.zeros(-(-N * PIX_BYTES // 128) * 128 // PIECE, bool)    # the line rule's bytes on the same frames: pieces in pairs
        lines[:N * npe] = marked
        line_total += int(lines.reshape(-1, 2).any(axis=1).sum()) * 128
    assert changed_total <= stored_total <= line_total
