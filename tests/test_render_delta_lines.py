"""The delta render's line rule on the host (babyai_amd/csrc/bbai_render.hpp, k_render_delta): a 128-byte line of the pixel
buffer is stored iff a cell it draws from changed its atlas tile id.  Checked against the reference's own frames (the golden pixel
traces) laid out back to back as the device buffer holds them: every line whose bytes differ from the previous frame is marked,
and storing only the marked lines over the previous frame gives the new frame -- across env boundaries (9408 = 73.5 lines)."""
import glob
import os

import numpy as np
import pytest

from hostsim_util import lib

PIX_BYTES, LINE, UNIT = 9408, 128, 8
GOLDEN = [p for p in sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))]


def cell_of_byte():
    """byte of an env's 56x56x3 image -> the cell (view x * 7 + view y) its tile comes from (k_render's render_chunk)."""
    b = np.arange(PIX_BYTES)
    py, cx = b // 168, (b % 168) // 24
    return cx * 7 + (py >> 3)


def line_table():
    """Per line of an 8-env unit: (first env, cells of it, cells of the next env) as k_render's delta prologue builds them."""
    cob = cell_of_byte()
    lea, ma, mb = [], [], []
    for l in range(UNIT * PIX_BYTES // LINE):
        b0, b1 = l * LINE, l * LINE + LINE
        ea, eb = b0 // PIX_BYTES, (b1 - 1) // PIX_BYTES
        end_a = (ea + 1) * PIX_BYTES if eb != ea else b1
        lea.append(ea)
        ma.append(set(cob[b0 - ea * PIX_BYTES:end_a - ea * PIX_BYTES].tolist()))
        mb.append(set(cob[0:b1 - eb * PIX_BYTES].tolist()) if eb != ea else set())
    return lea, ma, mb


def tile_ids(frames):
    """uint8[N, 56, 56, 3] -> int[N, 49]: one id per distinct 8x8 tile content (what the atlas id stands for)."""
    t = frames.reshape(len(frames), 7, 8, 7, 8, 3).transpose(0, 3, 1, 2, 4, 5).reshape(len(frames), 49, 192)
    _, ids = np.unique(t.reshape(-1, 192), axis=0, return_inverse=True)
    return ids.reshape(len(frames), 49)


def test_line_table_covers_every_byte_once():
    lea, ma, mb = line_table()
    assert len(lea) == 588 and max(lea) == 7
    cob = cell_of_byte()
    for l in range(588):                      # the marked cells are exactly the cells of the line's bytes
        buf = np.arange(l * LINE, l * LINE + LINE)
        env, off = buf // PIX_BYTES, buf % PIX_BYTES
        assert {(int(e), int(c)) for e, c in zip(env, cob[off])} == {(lea[l], c) for c in ma[l]} | {(lea[l] + 1, c) for c in mb[l]}
    assert sum(1 for m in mb if m) == 4       # an odd env starts mid-line: 4 lines of a unit span two envs


def test_line_table_is_the_headers():
    """The numpy table above against line_cells of bbai_render.hpp, called as init_line_table calls it: all 588 lines of a unit."""
    L = lib()
    lea, ma, mb = line_table()
    bits = lambda cells: sum(1 << c for c in cells)
    for l in range(588):
        b0, b1 = l * LINE, l * LINE + LINE
        ea, eb = b0 // PIX_BYTES, (b1 - 1) // PIX_BYTES
        assert ea == lea[l]
        assert L.hs_line_cells(b0 - ea * PIX_BYTES, ((ea + 1) * PIX_BYTES if eb != ea else b1) - ea * PIX_BYTES) == bits(ma[l]), l
        assert (L.hs_line_cells(0, b1 - eb * PIX_BYTES) if eb != ea else 0) == bits(mb[l]), l


@pytest.mark.parametrize("path", [p for p in GOLDEN if os.path.basename(p) in ("BossLevel.npz", "GoToLocal.npz")])      # (the traces with pixel frames)
def test_line_rule_against_brute_force(path):
    with np.load(path, allow_pickle=False) as f:
        pix = f["pixels"]
    assert pix.shape[1] > 0
    T, N = pix.shape[:2]
    lea, ma, mb = line_table()
    ids = tile_ids(pix.reshape(T * N, 56, 56, 3)).reshape(T, N, 49)
    n_pad = -(-N // UNIT) * UNIT
    flat_len = N * PIX_BYTES
    marked_total = changed_total = 0
    for t in range(1, T):
        prev, cur = pix[t - 1].reshape(-1), pix[t].reshape(-1)
        dirty_cells = np.zeros((n_pad, 49), bool)
        dirty_cells[:N] = ids[t] != ids[t - 1]
        n_lines = -(-flat_len // LINE)
        marked = np.zeros(n_lines, bool)
        for L in range(n_lines):
            u, l = divmod(L, 588)
            ea = u * UNIT + lea[l]
            marked[L] = any(dirty_cells[ea, c] for c in ma[l]) or any(dirty_cells[ea + 1, c] for c in mb[l])
        pad = n_lines * LINE - flat_len
        diff = np.concatenate([prev != cur, np.zeros(pad, bool)]).reshape(n_lines, LINE).any(axis=1)
        assert not (diff & ~marked).any(), t          # every changed line is stored
        out = prev.copy()
        for L in np.nonzero(marked)[0]:
            out[L * LINE:min((L + 1) * LINE, flat_len)] = cur[L * LINE:min((L + 1) * LINE, flat_len)]
        assert np.array_equal(out, cur), t
        marked_total += int(marked.sum())
        changed_total += int(diff.sum())
    assert changed_total <= marked_total < 2 * changed_total + 1      # (a changed tile id can leave some of its lines' bytes equal)
