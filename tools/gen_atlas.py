#!/usr/bin/env python3
"""Generate the tile atlases of the agent's 7x7 view (RGBImgPartialObsWrapper path): the 8-pixel one used by the k_render
kernels, the 16- and 32-pixel ones used by k_view_pixels.

Tiles are rasterised by the ORACLE's restated gym_minigrid renderer
(oracle/shim/gym_minigrid/minigrid.py Grid.render_tile, 3x supersampling) and
written to babyai_amd/data/tile_atlas_ts<size>.npz; the product only loads the files.  The tile-size-8 file is tracked; the 16 and 32
ones are build products (build() runs this tool) whose arrays tests/golden/view_atlas/ pins.
Re-run:  python tools/gen_atlas.py [--tile-size 8|16|32]      (default 8)

Layout: tiles uint8[n_tiles, ts, ts, 3]; lut uint8[2, 256] indexed by
key = type | colour << 3 | state << 6 of the encoded observation cell
(lut[0] = ordinary view cell, lut[1] = the agent's own cell (3,6) which shows the carried
object under the agent triangle).  Unknown keys map to tile 0 (unseen / un-highlighted empty).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refenv  # noqa: E402

refenv.enable_shim()
from gym_minigrid.minigrid import (COLOR_TO_IDX, IDX_TO_COLOR, OBJECT_TO_IDX, Grid, WorldObj)  # noqa: E402


def atlas(ts=8):
    """(tiles uint8[n_tiles, ts, ts, 3], lut uint8[2, 256]) at tile size `ts`."""
    def tile_u8(obj, agent_dir, highlight):
        t = Grid.render_tile(obj, agent_dir=agent_dir, highlight=highlight, tile_size=ts)
        out = np.zeros((ts, ts, 3), dtype=np.uint8)
        out[:, :, :] = t          # same float -> uint8 assignment as Grid.render
        return out

    tiles = [tile_u8(None, None, False)]          # tile 0: unseen
    lut = np.zeros((2, 256), dtype=np.uint8)

    def add(t):
        tiles.append(t)
        return len(tiles) - 1

    def key(t, c, s):
        return t | (c << 3) | (s << 6)

    # ordinary visible cells (always highlighted: the wrapper highlights exactly the visible mask)
    lut[0, key(OBJECT_TO_IDX['empty'], 0, 0)] = add(tile_u8(None, None, True))
    lut[0, key(OBJECT_TO_IDX['wall'], COLOR_TO_IDX['grey'], 0)] = add(
        tile_u8(WorldObj.decode(OBJECT_TO_IDX['wall'], COLOR_TO_IDX['grey'], 0), None, True))
    for name in ('key', 'ball', 'box'):
        for c in range(6):
            lut[0, key(OBJECT_TO_IDX[name], c, 0)] = add(tile_u8(WorldObj.decode(OBJECT_TO_IDX[name], c, 0), None, True))
    for c in range(6):
        for s in range(3):
            lut[0, key(OBJECT_TO_IDX['door'], c, s)] = add(tile_u8(WorldObj.decode(OBJECT_TO_IDX['door'], c, s), None, True))
    # the agent's cell: carried object (or nothing) + agent triangle pointing up (dir 3), highlighted
    lut[1, :] = add(tile_u8(None, 3, True))
    lut[1, key(OBJECT_TO_IDX['empty'], 0, 0)] = lut[1, 0]
    for name in ('key', 'ball', 'box'):
        for c in range(6):
            lut[1, key(OBJECT_TO_IDX[name], c, 0)] = add(tile_u8(WorldObj.decode(OBJECT_TO_IDX[name], c, 0), 3, True))
    return np.stack(tiles), lut


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument('--tile-size', type=int, default=8, choices=(8, 16, 32))
    args = ap.parse_args()
    tiles, lut = atlas(args.tile_size)
    out = os.path.join(ROOT, 'babyai_amd', 'data', 'tile_atlas_ts%d.npz' % args.tile_size)
    np.savez_compressed(out, tiles=tiles, lut=lut)
    print('wrote', out, tiles.shape, 'tiles')


if __name__ == '__main__':
    main()
