"""The tile atlases of the agent's 7x7 view (tools/gen_atlas.py): the tracked tile-size-8 file (babyai_amd/data/tile_atlas_ts8.npz) and the
pinned 16 / 32 arrays (tests/golden/view_atlas/) are what the tool's recipe regenerates from the oracle's Grid.render_tile, the files
build() writes next to the tile-size-8 one hold the pinned arrays, and frames gathered from them by the frame rule -- tile
lut[cell == (3, 6)][type | colour << 3 | state << 6] of view cell (x, y) at pixel rows y ts .., columns x ts .. -- are
RGBImgPartialObsWrapper(env, tile_size).observation of the oracle, byte for byte."""
import os
import sys

import numpy as np
import pytest

from oracle import refenv
from oracle import levels as olevels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
DATA = os.path.join(ROOT, "babyai_amd", "data", "tile_atlas_ts%d.npz")            # what the product loads (16 / 32: written by build())
GOLDEN = os.path.join(ROOT, "tests", "golden", "view_atlas", "tile_atlas_ts%d.npz")
LEVELS = ("BossLevel", "PickupLoc", "PutNextS5N2Carrying", "KeyCorridorS3R1", "GoToLocal", "UnlockPickup")


def load_atlas(ts):
    """(tiles, lut) of the tracked arrays: the tile-size-8 data file, the pinned copies at 16 / 32."""
    with np.load((DATA if ts == 8 else GOLDEN) % ts) as f:
        return f["tiles"], f["lut"]


def view_frames(image, tiles, lut, ts):
    """The frame rule in numpy: image uint8[k, 7, 7, 3] (indexed [x][y]) -> uint8[k, 7 ts, 7 ts, 3]."""
    image = np.asarray(image).reshape(-1, 7, 7, 3).astype(np.int64)
    key = (image[..., 0] | image[..., 1] << 3 | image[..., 2] << 6) & 255          # [k, x, y]
    row = np.zeros((7, 7), np.int64)
    row[3, 6] = 1
    ids = lut[row[None], key]                                                       # [k, x, y]
    fr = tiles[ids]                                                                 # [k, x, y, ts, ts, 3]
    return np.ascontiguousarray(fr.transpose(0, 2, 3, 1, 4, 5)).reshape(-1, 7 * ts, 7 * ts, 3)


@pytest.fixture(scope="module")
def gen_atlas():
    import gen_atlas
    return gen_atlas


@pytest.mark.parametrize("ts", [8, 16, 32])
def test_tracked_atlas_is_what_the_recipe_regenerates(gen_atlas, ts):
    tiles, lut = gen_atlas.atlas(ts)
    have_t, have_l = load_atlas(ts)
    assert tiles.shape == (58, ts, ts, 3) and tiles.dtype == np.uint8 and lut.shape == (2, 256) and lut.dtype == np.uint8
    assert np.array_equal(have_t, tiles) and have_t.dtype == np.uint8
    assert np.array_equal(have_l, lut) and have_l.dtype == np.uint8
    assert int(lut.max()) < len(tiles)


@pytest.mark.parametrize("ts", [16, 32])
def test_build_writes_the_pinned_arrays(ts):
    """What the product loads at 16 / 32 is a build product: build() leaves it in babyai_amd/data/ with the pinned arrays."""
    import __graft_entry__
    __graft_entry__.build()
    with np.load(DATA % ts) as f:
        tiles, lut = f["tiles"], f["lut"]
    want_t, want_l = load_atlas(ts)
    assert tiles.dtype == np.uint8 and np.array_equal(tiles, want_t)
    assert lut.dtype == np.uint8 and np.array_equal(lut, want_l)


def test_the_three_luts_are_one():
    """The lut does not depend on the tile size: the same keys name the same tile numbers."""
    l8 = load_atlas(8)[1]
    for ts in (16, 32):
        assert np.array_equal(load_atlas(ts)[1], l8)


def test_frame_rule_equals_the_oracle_wrapper():
    refenv.enable_shim()
    from gym_minigrid.wrappers import RGBImgPartialObsWrapper
    atl = {ts: load_atlas(ts) for ts in (16, 32)}
    frames = carried = doors = 0
    for name in LEVELS:
        e = olevels.make_env(name)
        wrap = {ts: RGBImgPartialObsWrapper(e, tile_size=ts) for ts in (16, 32)}
        rng = np.random.RandomState(1)
        for seed in range(3):
            e.seed(100 + seed)
            obs = e.reset()
            for t in range(60):
                for ts in (16, 32):
                    want = wrap[ts].observation(obs)["image"]
                    got = view_frames(obs["image"], *atl[ts], ts)[0]
                    assert want.shape == (7 * ts, 7 * ts, 3) and np.array_equal(got, want), (name, seed, t, ts)
                frames += 1
                carried += e.carrying is not None
                doors += bool((obs["image"][:, :, 0] == 4).any())
                obs, _, d, _ = e.step(rng.choice([0, 1, 2, 2, 2, 3, 4, 5]))
                if d:
                    obs = e.reset()
    assert frames == 1080 and carried >= 1 and doors >= 1, (frames, carried, doors)
