"""A plain reference of the partial-view pixel frame and of what a delta render of it must store, written from the
image geometry alone: pixel (y, x) of the 56x56 frame shows view cell (x // 8) * 7 + y // 8, the agent stands in cell 27, a cell's tile
comes from the atlas file (tiles[58, 8, 8, 3], lut[2, 256]: table 1 for the agent's cell, key = o0 | o1 << 3 | o2 << 6).  Nothing here
restates the kernels' chunk or line arithmetic.  tile_ids, frames and stored_mask take numpy arrays or torch tensors (the large GPU case
builds its reference on the device); everything else is numpy on the host.  Test harness only."""
import os

import numpy as np

VIEW, TILE, PIX = 7, 8, 56
CELLS, AGENT_CELL = VIEW * VIEW, 27
PIX_BYTES = PIX * PIX * 3
ATLAS_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "babyai_amd", "data", "tile_atlas_ts8.npz")

# Every (type, colour, state) cell the engine can emit (tests/test_gpu_parity.py::test_render_every_tile_vs_oracle: its `cells` and, for
# the agent's own cell, its `carried`): unseen, empty, wall, keys / balls / boxes in 6 colours, doors in 6 colours and 3 states.
ORDINARY = [(0, 0, 0), (1, 0, 0), (2, 5, 0)] + [(t, c, 0) for t in (5, 6, 7) for c in range(6)] + [(4, c, s) for c in range(6) for s in range(3)]
CARRIED = [(1, 0, 0)] + [(t, c, 0) for t in (5, 6, 7) for c in range(6)]
assert len(ORDINARY) == 39 and len(CARRIED) == 19

EVEN_SHARED = (4 * VIEW + 6, 5 * VIEW + 6, 6 * VIEW + 6)      # the cells of an even env's last 64 bytes: (4,6), (5,6), (6,6)
ODD_SHARED = (0 * VIEW + 0, 1 * VIEW + 0, 2 * VIEW + 0)       # the cells of an odd env's first 64 bytes: (0,0), (1,0), (2,0)
LAST_CELL = 6 * VIEW + 6                                      # (6,6): the cell of a frame's last byte

_atlas = {}


def atlas():
    """(tiles uint8[58, 8, 8, 3], lut uint8[2, 256]) of the shipped atlas file."""
    if "np" not in _atlas:
        with np.load(ATLAS_PATH) as f:
            _atlas["np"] = (np.ascontiguousarray(f["tiles"], dtype=np.uint8), np.ascontiguousarray(f["lut"], dtype=np.uint8))
        assert _atlas["np"][0].shape[1:] == (TILE, TILE, 3) and _atlas["np"][1].shape == (2, 256)
    return _atlas["np"]


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _atlas_like(x):
    """The atlas as arrays of x's kind (numpy, or torch on x's device)."""
    if not _is_torch(x):
        return atlas()
    key = str(x.device)
    if key not in _atlas:
        import torch
        _atlas[key] = tuple(torch.as_tensor(a, device=x.device) for a in atlas())
    return _atlas[key]


def _long(x):
    import torch
    return x.to(torch.int64) if _is_torch(x) else x.astype(np.int64)


def tile_ids(enc):
    """uint8[N, 7, 7, 3] (enc[n, x, y] = view cell 7 x + y) -> uint8[N, 49]: the atlas tile of every cell."""
    _, lut = _atlas_like(enc)
    e = _long(enc.reshape(len(enc), CELLS, 3))
    key = e[:, :, 0] | (e[:, :, 1] << 3) | (e[:, :, 2] << 6)
    assert int(key.max()) < 256, "an encoding the engine cannot emit (its key lies past the lut)"
    ids = lut[0][key]
    ids[:, AGENT_CELL] = lut[1][key[:, AGENT_CELL]]
    return ids


def frames(ids):
    """uint8[N, 49] -> uint8[N, 56, 56, 3]: pixel (y, x) = pixel (y % 8, x % 8) of the tile of cell (x // 8) * 7 + y // 8."""
    tiles, _ = _atlas_like(ids)
    n = len(ids)
    t = tiles[_long(ids)].reshape(n, VIEW, VIEW, TILE, TILE, 3)        # [n, cell x, cell y, y in tile, x in tile, rgb]
    t = t.permute(0, 2, 3, 1, 4, 5) if _is_torch(t) else t.transpose(0, 2, 3, 1, 4, 5)
    return t.reshape(n, PIX, PIX, 3)                                   # [n, (cell y, y in tile), (cell x, x in tile), rgb]


def cell_of_byte():
    """int[9408]: the view cell that byte b of a frame shows (byte b is a colour of pixel b // 3 = 56 y + x)."""
    p = np.arange(PIX_BYTES) // 3
    y, x = p // PIX, p % PIX
    return (x // TILE) * VIEW + y // TILE


def stored_mask_of(dirty, unit):
    """stored_mask from the dirty cells themselves, bool[N, 49]."""
    assert unit in (64, 128)
    n = len(dirty)
    cob = cell_of_byte()
    if _is_torch(dirty):
        import torch
        cob = torch.as_tensor(cob, device=dirty.device)
        touched = dirty[:, cob].reshape(-1)                            # per byte of the buffer: its cell changed
        pad = (-len(touched)) % unit                                   # (unit 128, odd N: the last line is half outside the buffer)
        if pad:
            touched = torch.cat([touched, torch.zeros(pad, dtype=torch.bool, device=dirty.device)])
        units = touched.reshape(-1, unit).any(dim=1)                   # units counted from the buffer's start
        return units.repeat_interleave(unit)[:n * PIX_BYTES]
    touched = dirty[:, cob].reshape(-1)
    pad = (-len(touched)) % unit
    touched = np.concatenate([touched, np.zeros(pad, bool)])
    units = touched.reshape(-1, unit).any(axis=1)
    return np.repeat(units, unit)[:n * PIX_BYTES]


def stored_fraction(dirty, unit):
    """stored_mask_of(dirty, unit).mean() at an eighth of the cost: cells, pieces and lines all start on multiples of 8 bytes."""
    n = len(dirty)
    touched = dirty[:, cell_of_byte()[::8]].reshape(-1)
    touched = np.concatenate([touched, np.zeros((-len(touched)) % (unit // 8), bool)])
    inside = np.arange(len(touched)) < n * PIX_BYTES // 8
    return float((np.repeat(touched.reshape(-1, unit // 8).any(axis=1), unit // 8) & inside).sum()) / (n * PIX_BYTES // 8)


def stored_mask(old_ids, new_ids, unit):
    """bool[N * 9408]: the bytes a delta render with render_piece_bytes = unit must write when the registered buffer holds the frame of
    old_ids and the new frame is new_ids'.  Unit 64: every 64-byte piece that contains a byte of a cell whose id changed (64 divides 9408:
    a piece lies inside one env).  Unit 128: every 128-byte line of the whole buffer, counted from its start, that contains such a byte of
    either env it touches (9408 = 73.5 lines: envs 2k and 2k + 1 share a line; only the bytes inside the buffer count)."""
    return stored_mask_of(old_ids != new_ids, unit)


# ---- synthetic inputs ---------------------------------------------------------------------------------------------------------------
def _keys(triples):
    a = np.asarray(triples, dtype=np.int64)
    return a[:, 0] | (a[:, 1] << 3) | (a[:, 2] << 6)


def _index_of_key(triples):
    """int[256]: key -> index in the list (-1: not in it)."""
    t = np.full(256, -1, np.int64)
    k = _keys(triples)
    assert len(set(k.tolist())) == len(k) and k.max() < 256
    t[k] = np.arange(len(k))
    return t


def synthetic_encodings(n, seed):
    """uint8[n, 7, 7, 3]: every ordinary cell a seeded draw from ORDINARY, the agent's cell CARRIED[(env + a seeded offset) % 19] -- 19
    consecutive envs hold every carried object."""
    rng = np.random.RandomState(seed)
    enc = np.asarray(ORDINARY, np.uint8)[rng.randint(0, len(ORDINARY), size=(n, CELLS))]
    enc[:, AGENT_CELL] = np.asarray(CARRIED, np.uint8)[(np.arange(n) + rng.randint(0, len(CARRIED))) % len(CARRIED)]
    return enc.reshape(n, VIEW, VIEW, 3)


def tiles_differ():
    """bool[58, 58]: do tiles a and b differ in a byte."""
    tiles, _ = atlas()
    flat = tiles.reshape(len(tiles), -1)
    return (flat[:, None, :] != flat[None, :, :]).any(axis=2)


def perturb(enc, pattern, seed=0):
    """enc with every cell of `pattern` (bool[N, 49], cell = 7 x + y) replaced by another entry of its list (ORDINARY; CARRIED for the
    agent's cell), a seeded choice.  Asserts what the tests rely on: exactly the pattern's cells change their tile id, and with it their
    tile's bytes."""
    n = len(enc)
    pattern = np.asarray(pattern, bool).reshape(n, CELLS)
    rng = np.random.RandomState(seed)
    out = enc.reshape(n, CELLS, 3).copy()
    key = _keys(out.reshape(-1, 3)).reshape(n, CELLS)
    hop = rng.randint(0, 1 << 30, size=(n, CELLS))
    for cols, triples in ((np.arange(CELLS) != AGENT_CELL, ORDINARY), (np.arange(CELLS) == AGENT_CELL, CARRIED)):
        sel = pattern & cols[None, :]
        cur = _index_of_key(triples)[key]                                # (-1: not an entry of the list -- any entry is another one)
        new = np.where(cur < 0, hop % len(triples), (cur + 1 + hop % (len(triples) - 1)) % len(triples))
        out[sel] = np.asarray(triples, np.uint8)[new[sel]]
    out = out.reshape(enc.shape)
    a, b = tile_ids(enc), tile_ids(out)
    assert np.array_equal(a != b, pattern), "perturb: the cells whose tile id changed are not the pattern's"
    assert tiles_differ()[a, b][pattern].all(), "perturb: a changed id with unchanged tile bytes"
    return out


# ---- dirty patterns by env index ----------------------------------------------------------------------------------------------------
# The catalogue, 57 kinds (odd: env i gets kind (i + shift) % 57, so every kind meets every position of a 32-env group, of an 8-env unit
# and of an even / odd pair within 57 x 32 envs): nothing; each single cell; all 49; only the three cells of an even env's last 64 bytes;
# nothing; only the three cells of an odd env's first 64 bytes; seeded subsets at densities 1/49, 1/8, 1/2.  "even-shared, nothing,
# odd-shared" in a row: where the first lands on an even env its pair is (dirty only in the shared line's cells, clean), where it lands on an
# odd one the next pair is (clean, dirty only in the shared line's cells).
KIND_NONE, KIND_ALL, KIND_EVEN_SHARED, KIND_NONE2, KIND_ODD_SHARED, KIND_R49, KIND_R8, KIND_R2, KINDS = 0, 50, 51, 52, 53, 54, 55, 56, 57


def single_kind(cell):
    return 1 + cell


def assign_patterns(n, shift, seed, clean_groups=()):
    """(pattern bool[n, 49], kind int[n]): env i gets kind (i + shift) % 57; the envs of the 32-env groups in `clean_groups` stay clean
    (kind -1); the last env of an odd n is dirty in cell (6,6) as well, whatever its kind, so that the buffer's last half line is written."""
    rng = np.random.RandomState(seed)
    kind = (np.arange(n) + shift) % KINDS
    pat = np.zeros((n, CELLS), bool)
    single = (kind >= 1) & (kind <= CELLS)
    pat[np.nonzero(single)[0], kind[single] - 1] = True
    pat[kind == KIND_ALL] = True
    pat[np.ix_(kind == KIND_EVEN_SHARED, EVEN_SHARED)] = True
    pat[np.ix_(kind == KIND_ODD_SHARED, ODD_SHARED)] = True
    u = rng.random_sample((n, CELLS))
    for k, density in ((KIND_R49, 1.0 / 49), (KIND_R8, 1.0 / 8), (KIND_R2, 1.0 / 2)):
        pat[kind == k] = u[kind == k] < density
    for g in clean_groups:
        pat[32 * g:32 * g + 32] = False
        kind[32 * g:32 * g + 32] = -1
    if n % 2:
        pat[n - 1, LAST_CELL] = True
    return pat, kind


def check_patterns(pat, kind, clean_groups=(), large=False, last_clean=False):
    """The preconditions a footprint case states about its own dirty patterns (conditions on the inputs, not measurements)."""
    n = len(pat)
    dirty_env = pat.any(axis=1)
    for unit in (64, 128):
        frac = stored_fraction(pat, unit)
        assert 0.01 <= frac <= 0.60, (unit, frac)                       # neither branch of the expected frame's `where` is vacuous
    if n % 2:
        assert pat[n - 1, LAST_CELL]
    if last_clean:
        assert n >= 2 and not dirty_env[n - 1] and dirty_env[n - 2]
    ngroups = -(-n // 32)
    group_dirty = np.array([dirty_env[32 * g:32 * g + 32].any() for g in range(ngroups)])
    for g in clean_groups:                                              # a whole clean group between two dirty ones
        assert 32 * g + 32 <= n and not group_dirty[g] and group_dirty[:g].any() and group_dirty[g + 1:].any(), g
    if not large:
        return
    env = np.arange(n)
    only = lambda cells: pat[:, list(cells)].all(axis=1) & (pat.sum(axis=1) == len(cells))
    for c in range(CELLS):                                              # every (env % 32, single dirty cell) pair
        assert len(set((env[only([c]) & (kind == single_kind(c))] % 32).tolist())) == 32, c
    assert len(set((env[pat.all(axis=1)] % 8).tolist())) == 8           # "all 49 cells" at every position of an 8-env unit
    ev, od = env[0:n - 1:2], env[1:n:2]
    assert (~dirty_env[ev] & only(ODD_SHARED)[od]).any()                # even env clean, odd env dirty only in its first-64-byte cells
    assert (only(EVEN_SHARED)[ev] & ~dirty_env[od]).any()               # ... and the mirror image
    assert len(clean_groups) > 0


# ---- the GPU cases' dirty patterns (tests/test_gpu_render_delta_footprint.py; their preconditions: tests/test_render_footprint_host.py) ----
class Case(object):
    """n envs; transition k (a delta render, or a step of the from-step protocol) takes assign_patterns(n, shifts[k], ...) with the groups
    clean[k] kept clean; last_clean[k]: the last env is clean there and the one before it dirty."""

    def __init__(self, n, shifts, clean=None, last_clean=(), large=False):
        self.n, self.shifts, self.large = n, list(shifts), large
        self.clean = clean if clean is not None else [()] * len(self.shifts)
        self.last_clean = set(last_clean)

    def patterns(self, k):
        return assign_patterns(self.n, self.shifts[k], 1000 * self.n + k, self.clean[k])

    def conditions(self, k):
        return dict(clean_groups=self.clean[k], large=self.large, last_clean=k in self.last_clean)


LARGE_N = 41061                                   # 1284 groups of 32 (the last one: 5 envs) over at most 256 blocks
_LARGE_CLEAN = tuple(range(2, LARGE_N // 32, 5))
CASES = [
    Case(1, [49, 1, 25]),
    Case(7, [47, 0, 20]),
    Case(8, [45, 50, 10], last_clean=[0]),
    Case(9, [46, 3, 51]),
    Case(31, [40, 10, 53]),
    Case(32, [30, 8, 52]),
    Case(33, [25, 50, 5]),
    Case(65, [28, 45, 50], clean=[(1,), (), (1,)]),
    Case(128 + 37, [0, 20, 40], clean=[(3,), (), (1, 3)]),
    Case(LARGE_N, [0, 31, 13], clean=[_LARGE_CLEAN] * 3, large=True),
]
CASE = {c.n: c for c in CASES}
