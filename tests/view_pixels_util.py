"""A plain reference of the partial-view pixel frame at any view size and tile size, written from the picture's geometry alone
(render_util.tile_ids / frames, with V and the tile size as arguments): a frame is uint8[V ts, V ts, 3]; pixel (row, column) shows view
cell (vi, vj) = (column // ts, row // ts), whose encoding is enc[vi, vj]; the agent stands in cell (V // 2, V - 1); a cell's tile comes
from the atlas files (tiles[58, ts, ts, 3], lut[2, 256]: table 1 for the agent's cell, key = o0 | o1 << 3 | o2 << 6).  Nothing here
restates the kernel's chunk or piece arithmetic.  tile_ids and frames take numpy arrays or torch tensors (the large GPU cases build
their reference on the device).  Test harness only."""
import os

import numpy as np

import render_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEW_SIZES = (3, 5, 7, 9, 11)
TILE_SIZES = (8, 16, 32)
ATLAS_FILES = {8: os.path.join(ROOT, "babyai_amd", "data", "tile_atlas_ts8.npz"),
               16: os.path.join(ROOT, "tests", "golden", "view_atlas", "tile_atlas_ts16.npz"),
               32: os.path.join(ROOT, "tests", "golden", "view_atlas", "tile_atlas_ts32.npz")}

_atlas = {}


def agent_cell(V):
    return (V // 2) * V + V - 1


def frame_bytes(V, ts):
    return 3 * V * V * ts * ts


def atlas(ts):
    """(tiles uint8[58, ts, ts, 3], lut uint8[2, 256]) of the atlas file of tile size ts."""
    if ts not in _atlas:
        with np.load(ATLAS_FILES[ts]) as f:
            _atlas[ts] = (np.ascontiguousarray(f["tiles"], dtype=np.uint8), np.ascontiguousarray(f["lut"], dtype=np.uint8))
        assert _atlas[ts][0].shape[1:] == (ts, ts, 3) and _atlas[ts][1].shape == (2, 256)
    return _atlas[ts]


def _atlas_like(x, ts):
    if not render_util._is_torch(x):
        return atlas(ts)
    key = (ts, str(x.device))
    if key not in _atlas:
        import torch
        _atlas[key] = tuple(torch.as_tensor(a, device=x.device) for a in atlas(ts))
    return _atlas[key]


def tile_ids(enc, ts):
    """uint8[N, V, V, 3] (enc[n, vi, vj] = view cell V vi + vj) -> uint8[N, V V]: the atlas tile of every cell."""
    V = enc.shape[1]
    assert tuple(enc.shape[1:]) == (V, V, 3)
    _, lut = _atlas_like(enc, ts)
    e = render_util._long(enc.reshape(len(enc), V * V, 3))
    key = e[:, :, 0] | (e[:, :, 1] << 3) | (e[:, :, 2] << 6)
    assert len(enc) == 0 or int(key.max()) < 256, "an encoding the engine cannot emit (its key lies past the lut)"
    ids = lut[0][key]
    ids[:, agent_cell(V)] = lut[1][key[:, agent_cell(V)]]
    return ids


def frames_of_ids(ids, V, ts):
    """uint8[N, V V] -> uint8[N, V ts, V ts, 3]: pixel (y, x) = pixel (y % ts, x % ts) of the tile of cell (x // ts) * V + y // ts."""
    tiles, _ = _atlas_like(ids, ts)
    n = len(ids)
    t = tiles[render_util._long(ids)].reshape(n, V, V, ts, ts, 3)          # [n, cell vi, cell vj, y in tile, x in tile, rgb]
    t = t.permute(0, 2, 3, 1, 4, 5) if render_util._is_torch(t) else t.transpose(0, 2, 3, 1, 4, 5)
    return t.reshape(n, V * ts, V * ts, 3)                                 # [n, (cell vj, y in tile), (cell vi, x in tile), rgb]


def frames(enc, ts):
    """uint8[N, V, V, 3] -> uint8[N, V ts, V ts, 3]."""
    return frames_of_ids(tile_ids(enc, ts), enc.shape[1], ts)


def synthetic_encodings(n, V, seed):
    """uint8[n, V, V, 3]: every ordinary cell a seeded draw from render_util.ORDINARY, the agent's cell CARRIED[(row + a seeded offset)
    % 19] -- 19 consecutive rows hold every carried object."""
    rng = np.random.RandomState(seed)
    enc = np.asarray(render_util.ORDINARY, np.uint8)[rng.randint(0, len(render_util.ORDINARY), size=(n, V * V))]
    enc[:, agent_cell(V)] = np.asarray(render_util.CARRIED, np.uint8)[(np.arange(n) + rng.randint(0, len(render_util.CARRIED))) % len(render_util.CARRIED)]
    return enc.reshape(n, V, V, 3)
