"""The reference side of tests/test_gpu_render_delta_footprint.py pinned without a GPU (tests/render_util.py): frames against the oracle's
own rasteriser, the stored-byte masks against the piece and line tables that tests/test_render_delta_pieces.py and
tests/test_render_delta_lines.py hold to the header's line_cells, hand-computed anchors, and the preconditions of every dirty pattern the
GPU cases use."""
import numpy as np
import pytest

import render_util as ru
from render_util import CELLS, PIX_BYTES
from test_render_delta_lines import line_table
from test_render_delta_pieces import piece_table


def cell(x, y):
    return 7 * x + y


def test_lists_map_to_distinct_tiles():
    """Within each list all entries have distinct tile ids with distinct tile contents: another entry is another id and other bytes."""
    tiles, lut = ru.atlas()
    assert tiles.shape == (58, 8, 8, 3) and lut.shape == (2, 256)
    differ = ru.tiles_differ()
    for table, triples in ((0, ru.ORDINARY), (1, ru.CARRIED)):
        ids = [int(lut[table][o0 | o1 << 3 | o2 << 6]) for o0, o1, o2 in triples]
        assert len(set(ids)) == len(ids) and max(ids) < len(tiles)
        for i in ids:
            for j in ids:
                assert differ[i, j] == (i != j)


def test_frames_equal_the_oracle_render():
    from oracle import levels as olevels
    n = 40
    enc = ru.synthetic_encodings(n, 5)
    seen = {tuple(x) for e in enc for k, x in enumerate(e.reshape(CELLS, 3)) if k != ru.AGENT_CELL}
    assert seen == set(ru.ORDINARY) and {tuple(e[3, 6]) for e in enc} == set(ru.CARRIED)
    pix = ru.frames(ru.tile_ids(enc))
    assert pix.shape == (n, 56, 56, 3) and pix.dtype == np.uint8
    ref_env = olevels.make_env("GoToLocal")
    for e in range(n):
        assert np.array_equal(pix[e], ref_env.get_obs_render(enc[e], tile_size=8)), e


def test_frames_pixel_by_pixel():
    """frames' reshape against the statement it implements, one pixel at a time."""
    tiles, _ = ru.atlas()
    ids = ru.tile_ids(ru.synthetic_encodings(3, 9))
    pix = ru.frames(ids)
    for y in range(56):
        for x in range(56):
            assert np.array_equal(pix[:, y, x], tiles[ids[:, (x // 8) * 7 + y // 8], y % 8, x % 8]), (y, x)


def test_torch_and_numpy_agree():
    import torch
    enc0 = ru.synthetic_encodings(9, 2)
    pat, _ = ru.assign_patterns(9, 47, 3)
    enc1 = ru.perturb(enc0, pat, seed=4)
    a, b = ru.tile_ids(enc0), ru.tile_ids(enc1)
    ta, tb = ru.tile_ids(torch.as_tensor(enc0)), ru.tile_ids(torch.as_tensor(enc1))
    assert np.array_equal(ta.numpy(), a) and np.array_equal(tb.numpy(), b) and ta.dtype == torch.uint8
    assert np.array_equal(ru.frames(tb).numpy(), ru.frames(b))
    for unit in (64, 128):
        assert np.array_equal(ru.stored_mask(ta, tb, unit).numpy(), ru.stored_mask(a, b, unit))


def test_perturb_changes_exactly_the_pattern():
    enc = ru.synthetic_encodings(57, 1)
    pat, kind = ru.assign_patterns(57, 0, 2)
    assert set(kind.tolist()) == set(range(ru.KINDS))
    out = ru.perturb(enc, pat, seed=3)
    changed = (out != enc).any(axis=3).reshape(57, CELLS)
    assert np.array_equal(changed, pat)
    allowed = set(ru.ORDINARY)
    for e in out:
        assert {tuple(x) for k, x in enumerate(e.reshape(CELLS, 3)) if k != ru.AGENT_CELL} <= allowed and tuple(e[3, 6]) in ru.CARRIED
    assert np.array_equal(ru.perturb(enc, np.zeros((57, CELLS), bool)), enc)
    with pytest.raises(AssertionError):
        ru.tile_ids(np.full((1, 7, 7, 3), 7, np.uint8))                  # key 511: past the lut


def random_dirty(n, seed):
    rng = np.random.RandomState(seed)
    d = rng.random_sample((n, CELLS)) < rng.choice([0.0, 0.02, 0.1, 0.5], size=(n, 1))
    for e in range(min(n, CELLS)):
        d[e, (e * 11) % CELLS] = True
    return d


@pytest.mark.parametrize("n", [1, 2, 9, 64])
def test_stored_mask_64_is_the_piece_table(n):
    table = piece_table()                                                 # [147, 49]
    dirty = random_dirty(n, n)
    marked = (dirty.astype(np.uint8) @ table.T.astype(np.uint8) > 0).reshape(-1)      # [n * 147], as test_piece_rule_against_brute_force
    assert np.array_equal(ru.stored_mask_of(dirty, 64), np.repeat(marked, 64))


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 33])
def test_stored_mask_128_is_the_line_table(n):
    lea, ma, mb = line_table()
    dirty = random_dirty(n, 100 + n)
    padded = np.zeros((-(-n // 8) * 8 + 1, CELLS), bool)
    padded[:n] = dirty
    n_lines = -(-n * PIX_BYTES // 128)
    marked = np.zeros(n_lines, bool)
    for L in range(n_lines):                                              # as test_line_rule_against_brute_force
        u, l = divmod(L, 588)
        ea = u * 8 + lea[l]
        marked[L] = any(padded[ea, c] for c in ma[l]) or any(padded[ea + 1, c] for c in mb[l])
    assert np.array_equal(ru.stored_mask_of(dirty, 128), np.repeat(marked, 128)[:n * PIX_BYTES])


def test_stored_mask_from_ids():
    old = ru.tile_ids(ru.synthetic_encodings(5, 3))
    new = old.copy()
    new[2, 30] ^= 1
    new[4, 0] ^= 1
    dirty = np.zeros((5, CELLS), bool)
    dirty[2, 30] = dirty[4, 0] = True
    for unit in (64, 128):
        m = ru.stored_mask(old, new, unit)
        assert m.shape == (5 * PIX_BYTES,) and m.dtype == bool and np.array_equal(m, ru.stored_mask_of(dirty, unit))
        assert not ru.stored_mask(old, old, unit).any()
        assert ru.stored_fraction(dirty, unit) == m.mean() > 0
        d3 = random_dirty(3, 8)
        assert ru.stored_fraction(d3, unit) == ru.stored_mask_of(d3, unit).mean()


def test_anchor_cell_0_0_pieces():
    """Cell (0,0) covers bytes row * 168 .. row * 168 + 23 of pixel rows 0..7: a change of it alone stores the 64-byte pieces those ranges
    meet.  By hand: row 0 -> piece 0; 168..191 -> 2; 336..359 -> 5; 504..527 -> 7 and 8; 672..695 -> 10; 840..863 -> 13; 1008..1031 -> 15
    and 16; 1176..1199 -> 18."""
    pieces = set()
    for row in range(8):
        for b in range(row * 168, row * 168 + 24):
            pieces.add(b // 64)
    assert pieces == {0, 2, 5, 7, 8, 10, 13, 15, 16, 18}
    dirty = np.zeros((3, CELLS), bool)
    dirty[1, cell(0, 0)] = True
    m = ru.stored_mask_of(dirty, 64).reshape(3, 147, 64)
    assert m.all(axis=2).sum() == m.any(axis=2).sum() == len(pieces)      # whole pieces
    assert set(np.nonzero(m[1].any(axis=1))[0].tolist()) == pieces and not m[0].any() and not m[2].any()


def test_anchor_shared_line_cells():
    """The line envs 2k and 2k + 1 share: the even env's last 64 bytes show cells (4,6), (5,6), (6,6), the odd env's first 64 bytes
    (0,0), (1,0), (2,0)."""
    assert PIX_BYTES % 128 == 64
    cob = ru.cell_of_byte()
    assert set(cob[PIX_BYTES - 64:].tolist()) == {cell(4, 6), cell(5, 6), cell(6, 6)} == set(ru.EVEN_SHARED)
    assert set(cob[:64].tolist()) == {cell(0, 0), cell(1, 0), cell(2, 0)} == set(ru.ODD_SHARED)
    assert cob[PIX_BYTES - 1] == ru.LAST_CELL == cell(6, 6)
    for k in (0, 1):                                                      # (pair 0 starts a unit of 8 envs, pair 1 does not)
        shared = slice((2 * k + 1) * PIX_BYTES - 64, (2 * k + 1) * PIX_BYTES + 64)
        assert shared.start % 128 == 0
        for env, cells in ((2 * k, ru.EVEN_SHARED), (2 * k + 1, ru.ODD_SHARED)):
            for c in cells:
                dirty = np.zeros((5, CELLS), bool)
                dirty[env, c] = True
                m128, m64 = ru.stored_mask_of(dirty, 128), ru.stored_mask_of(dirty, 64)
                assert m128[shared].all()                                 # the whole line, the clean neighbour's half included
                half = slice(shared.start, shared.start + 64) if env % 2 == 0 else slice(shared.start + 64, shared.stop)
                other = slice(shared.start + 64, shared.stop) if env % 2 == 0 else slice(shared.start, shared.start + 64)
                assert m64[half].all() and not m64[other].any()           # pieces stay inside their env
                clean = np.ones(5 * PIX_BYTES, bool)
                clean[env * PIX_BYTES:(env + 1) * PIX_BYTES] = False
                clean[shared] = False
                assert not m128[clean].any() and not m64[clean].any()


def test_odd_batch_ends_in_half_a_line():
    dirty = np.zeros((3, CELLS), bool)
    dirty[2, ru.LAST_CELL] = True
    m = ru.stored_mask_of(dirty, 128)
    assert len(m) == 3 * PIX_BYTES and len(m) % 128 == 64 and m[-64:].all() and not m[:2 * PIX_BYTES].any()


def test_pattern_catalogue():
    pat, kind = ru.assign_patterns(57, 0, 7)
    assert not pat[ru.KIND_NONE].any() and not pat[ru.KIND_NONE2].any() and pat[ru.KIND_ALL].all()
    for c in range(CELLS):
        assert np.array_equal(np.nonzero(pat[ru.single_kind(c)])[0], [c])
    assert set(np.nonzero(pat[ru.KIND_EVEN_SHARED])[0].tolist()) == set(ru.EVEN_SHARED)
    assert set(np.nonzero(pat[ru.KIND_ODD_SHARED])[0].tolist()) == set(ru.ODD_SHARED)
    assert (ru.KIND_EVEN_SHARED + 1, ru.KIND_ODD_SHARED - 1) == (ru.KIND_NONE2, ru.KIND_NONE2)
    big, _ = ru.assign_patterns(57 * 40, 0, 7)
    for k, density in ((ru.KIND_R49, 1 / 49.0), (ru.KIND_R8, 1 / 8.0), (ru.KIND_R2, 1 / 2.0)):
        rows = big[k::57]
        assert 0.5 * density < rows.mean() < 1.5 * density and len({r.tobytes() for r in rows}) > 1


@pytest.mark.parametrize("case", ru.CASES, ids=lambda c: "n%d" % c.n)
def test_gpu_cases_meet_their_preconditions(case):
    """Every transition of every GPU case, built exactly as the GPU tests build it."""
    assert len(case.shifts) >= 3
    for k in range(len(case.shifts)):
        pat, kind = case.patterns(k)
        ru.check_patterns(pat, kind, **case.conditions(k))
    assert any(c.n % 2 == 0 and c.conditions(k)["last_clean"] for c in ru.CASES for k in range(len(c.shifts)))
    assert {c.n for c in ru.CASES} >= {1, 7, 8, 9, 31, 32, 33, 65, 128 + 37, 41061}
