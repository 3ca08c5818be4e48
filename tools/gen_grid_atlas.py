#!/usr/bin/env python3
"""Generate the tile atlases of the full-grid picture, MiniGridEnv.render('rgb_array', highlight, tile_size) (k_render_grid).

Tiles are rasterised by the ORACLE's restated gym_minigrid renderer (oracle/shim/gym_minigrid/minigrid.py Grid.render_tile,
3x supersampling, then the same float -> uint8 assignment as Grid.render).  __graft_entry__.build() runs this tool to write the
product's copies, babyai_amd/data/grid_atlas_ts{8,16,32}.npz (build products, not tracked); the product only loads them.  The same
arrays are pinned as test vectors in tests/golden/grid_atlas/*.npz (tests/test_grid_render_host.py).
    python tools/gen_grid_atlas.py [--out DIR]        (default: babyai_amd/data)

Layout: tiles uint8[n_tiles, ts, ts, 3]; lut uint8[2, 5, 256] indexed by [highlight][agent][key], agent = 0 (no agent on the
cell) or 1 + the agent's direction, key = type | colour << 3 | state << 6 = the record plane's appearance byte.  Every cell a
grid can hold has a tile: empty, the grey wall, key / ball / box x 6 colours, door x 6 colours x 3 states, and the agent
(4 directions) on an empty cell or on an open door -- each with and without highlight.  Keys no grid can hold map to tile 0.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refenv  # noqa: E402

refenv.enable_shim()
from gym_minigrid.minigrid import COLOR_TO_IDX, OBJECT_TO_IDX, Grid, WorldObj  # noqa: E402

TILE_SIZES = (8, 16, 32)


def key(t, c, s):
    return t | (c << 3) | (s << 6)


def grid_cells():
    """(key, WorldObj or None) of every cell a BabyAI grid can hold."""
    out = [(key(OBJECT_TO_IDX['empty'], 0, 0), None),
           (key(OBJECT_TO_IDX['wall'], COLOR_TO_IDX['grey'], 0), WorldObj.decode(OBJECT_TO_IDX['wall'], COLOR_TO_IDX['grey'], 0))]
    for name in ('key', 'ball', 'box'):
        for c in range(6):
            out.append((key(OBJECT_TO_IDX[name], c, 0), WorldObj.decode(OBJECT_TO_IDX[name], c, 0)))
    for c in range(6):
        for s in range(3):
            out.append((key(OBJECT_TO_IDX['door'], c, s), WorldObj.decode(OBJECT_TO_IDX['door'], c, s)))
    return out


def agent_cells():
    """The cells the agent can stand on: empty, or an open door."""
    return [(k, o) for k, o in grid_cells() if o is None or (o.type == 'door' and (k >> 6) == 0)]


def build(ts):
    tiles = []
    lut = np.zeros((2, 5, 256), dtype=np.uint8)

    def tile(obj, agent_dir, hl):
        t = Grid.render_tile(obj, agent_dir=agent_dir, highlight=hl, tile_size=ts)
        out = np.zeros((ts, ts, 3), dtype=np.uint8)
        out[:, :, :] = t          # same float -> uint8 assignment as Grid.render
        tiles.append(out)
        return len(tiles) - 1

    for hl in (0, 1):
        for k, obj in grid_cells():
            lut[hl, 0, k] = tile(obj, None, bool(hl))
        for d in range(4):
            for k, obj in agent_cells():
                lut[hl, 1 + d, k] = tile(obj, d, bool(hl))
    return np.stack(tiles), lut


def path(ts, out_dir=None):
    return os.path.join(out_dir or os.path.join(ROOT, 'babyai_amd', 'data'), 'grid_atlas_ts%d.npz' % ts)


def main():
    out_dir = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else None
    for ts in TILE_SIZES:
        tiles, lut = build(ts)
        dst = path(ts, out_dir)
        tmp = '%s.tmp%d.npz' % (dst[:-4], os.getpid())      # written under a private name and renamed: concurrent builds never see half a file
        np.savez_compressed(tmp, tiles=tiles, lut=lut)
        os.replace(tmp, dst)
        print('wrote', dst, tiles.shape, 'tiles')


if __name__ == '__main__':
    main()
