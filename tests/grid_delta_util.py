"""The reference side of the full-grid delta render's tests (k_grid_delta, include/bbai_grid_target.h), written from the picture's geometry
alone -- not from babyai_amd/csrc/bbai_gridtarget.hpp, which tests/test_grid_delta_host.py holds against this file.

A frame is uint8[H ts][W ts][3], row-major: H ts pixel rows of RB = 3 W ts bytes.  Byte b lies in pixel row b // RB, so in tile row
(b // RB) // ts, and in column (b % RB) // (3 ts).  The store unit is the 64-byte piece: piece p = bytes [64 p, 64 p + 64).  A piece is
dirty iff one of its bytes lies in a cell whose tile id changed."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECE = 64
TILE_SIZES = (8, 16, 32)
_cache = {}


def frame_bytes(W, H, ts):
    return 3 * W * H * ts * ts


def byte_cells(W, H, ts):
    """(tile row y, column x) of every byte of a frame, int32[F] each."""
    b = np.arange(frame_bytes(W, H, ts), dtype=np.int64)
    rb = 3 * W * ts
    return ((b // rb) // ts).astype(np.int32), ((b % rb) // (3 * ts)).astype(np.int32)


def piece_cells(W, H, ts):
    """bool[NP, H * W]: piece p holds a byte of cell y * W + x."""
    key = ("pc", W, H, ts)
    if key not in _cache:
        y, x = byte_cells(W, H, ts)
        assert len(y) % PIECE == 0
        npieces = len(y) // PIECE
        inc = np.zeros((npieces, H * W), bool)
        inc[np.repeat(np.arange(npieces), PIECE), y.astype(np.int64) * W + x] = True
        _cache[key] = inc
    return _cache[key]


def piece_segments(W, H, ts):
    """Every piece's segments as (n, y0, cols0, y1, cols1): the tile rows it holds bytes of (one or two, the second -1 / 0 where there is
    one) and, per tile row, the mask of the columns it holds bytes of."""
    inc = piece_cells(W, H, ts).reshape(-1, H, W)
    weights = (1 << np.arange(W, dtype=np.int64))
    rowmask = (inc * weights[None, None, :]).sum(axis=2)               # [NP, H]
    has = rowmask != 0
    n = has.sum(axis=1)
    assert n.min() >= 1 and n.max() <= 2
    y0 = has.argmax(axis=1)
    y1 = np.where(n == 2, H - 1 - has[:, ::-1].argmax(axis=1), -1)
    assert ((y1 == -1) | (y1 == y0 + 1)).all()
    idx = np.arange(len(n))
    return n, y0, rowmask[idx, y0], y1, np.where(n == 2, rowmask[idx, np.maximum(y1, 0)], 0)


def stored_mask(ids_before, ids_after, W, H, ts):
    """bool[n, NP]: the pieces of every env's frame a delta render from `ids_before` to `ids_after` (uint8[n, H * W], row-major) has to
    store -- those that hold a byte of a changed cell -- and no others."""
    changed = (np.asarray(ids_before) != np.asarray(ids_after)).reshape(-1, H * W)
    inc = piece_cells(W, H, ts)
    return (changed.astype(np.float32) @ inc.T.astype(np.float32)) > 0


def atlas(ts):
    """(tiles uint8[T, ts, ts, 3], lut uint8[2, 5, 256]) of the full-grid picture at tile size ts (a build product)."""
    key = ("atlas", ts)
    if key not in _cache:
        with np.load(os.path.join(ROOT, "babyai_amd", "data", "grid_atlas_ts%d.npz" % ts)) as f:
            tiles, lut = np.ascontiguousarray(f["tiles"], dtype=np.uint8), np.ascontiguousarray(f["lut"], dtype=np.uint8)
        flat = tiles.reshape(len(tiles), -1)
        assert len(np.unique(flat, axis=0)) == len(flat), "the atlas tiles are not pairwise distinct"
        _cache[key] = (tiles, lut.reshape(2, 5, 256))
    return _cache[key]


def frames_of_ids(ids, W, H, ts):
    """uint8[n, H ts, W ts, 3] of tile ids uint8[n, H * W]."""
    tiles, _ = atlas(ts)
    n = len(ids)
    return np.ascontiguousarray(tiles[np.asarray(ids).reshape(n, H, W)].transpose(0, 1, 3, 2, 4, 5)).reshape(n, H * ts, W * ts, 3)


def frame_ids(frame, atlas_tiles):
    """Tile ids uint8[n, H * W] of frames uint8[n, H ts, W ts, 3]: each cell's ts x ts x 3 block looked up in the atlas (every block must be
    a tile of it; the tiles are pairwise distinct, atlas())."""
    tiles = np.asarray(atlas_tiles)
    ts = tiles.shape[1]
    n, hp, wp, _ = frame.shape
    H, W = hp // ts, wp // ts
    flat = tiles.reshape(len(tiles), -1)
    assert len(np.unique(flat, axis=0)) == len(flat), "the atlas tiles are not pairwise distinct"
    blocks = np.ascontiguousarray(np.asarray(frame).reshape(n, H, ts, W, ts, 3).transpose(0, 1, 3, 2, 4, 5)).reshape(n * H * W, -1)
    where = {t.tobytes(): i for i, t in enumerate(flat)}
    uniq, inv = np.unique(blocks, axis=0, return_inverse=True)
    ids = np.array([where[u.tobytes()] for u in uniq], np.uint8)       # (KeyError: a block that is no tile)
    return ids[inv.reshape(-1)].reshape(n, H * W)


def probe_positions(ts):
    """A few byte positions of a tile that tell every atlas tile from every other (chosen greedily): what the device-side lookup reads."""
    key = ("probe", ts)
    if key not in _cache:
        flat = atlas(ts)[0].reshape(-1, 3 * ts * ts).astype(np.int64)
        pos, groups = [], np.zeros(len(flat), np.int64)
        while len(np.unique(groups)) < len(flat):
            best = max(range(flat.shape[1]), key=lambda p: len(np.unique(groups * 256 + flat[:, p])))
            pos.append(best)
            groups = np.unique(groups * 256 + flat[:, best], return_inverse=True)[1].reshape(-1)
        _cache[key] = np.array(pos, np.int64)
    return _cache[key]


def frame_ids_device(frame, ts):
    """frame_ids on the device (torch): the ids from probe_positions' bytes of every block, then EVERY byte of every block held against
    that tile of the atlas -- the same lookup, without a host copy of the frames (BossLevel at 32: 1.49 MB per env)."""
    import torch
    tiles = torch.as_tensor(atlas(ts)[0], device=frame.device)
    n, hp, wp, _ = frame.shape
    H, W = hp // ts, wp // ts
    blocks = frame.reshape(n, H, ts, W, ts, 3).permute(0, 1, 3, 2, 4, 5)                 # [n, H, W, ts, ts, 3]
    pos = torch.as_tensor(probe_positions(ts), device=frame.device)
    py, px, pc = pos // (3 * ts), (pos // 3) % ts, pos % 3
    got = blocks[:, :, :, py, px, pc].reshape(-1, len(pos))                             # [cells, K]
    want = tiles.reshape(len(tiles), -1)[:, pos]                                        # [T, K]
    match = (got[:, None, :] == want[None, :, :]).all(dim=2)
    assert bool(match.any(dim=1).all()), "a block that is no tile of the atlas"
    ids = match.to(torch.uint8).argmax(dim=1).to(torch.uint8).reshape(n, H * W)
    assert torch.equal(tiles[ids.reshape(n, H, W).long()], blocks), "a block that is no tile of the atlas"
    return ids


def level_grids():
    """{(W, H)} of the 105 levels."""
    from babyai_amd import levels
    out = set()
    for name in levels.LEVELS:
        c = levels.make_cfg("BabyAI-%s-v0" % name)
        out.add((int(c.W), int(c.H)))
    return out
