"""Host side of the batched BabyAI engine: ctypes binding of the C ABI (include/bbai.h)
over torch device tensors.

`BatchedBabyAIEnv` exposes the reference's env protocol in batched / tensor form:
`seed(seeds)`, `reset() -> obs`, `step(actions) -> (obs, reward, done, info)` with the same
`{image, direction, mission}` observation dict (reference: babyai/levels/levelgen.py:35-66,
obs keys babyai/utils/demos.py:57-59).  The list-of-dicts adapters that plug into the
reference's `ParallelEnv` / `ManyEnvs` call sites live in babyai_amd/vec_env.py.

PyTorch is used only for device memory, streams and (in bench.py) torch.distributed.
There is NO CPU fallback: if the HIP library is missing or no GPU is visible, construction
raises.
"""
import ctypes
import sys
import os

import numpy as np

from .levels import level_name, make_cfg
from . import missions

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BBAI_ENGINE_LIB") or os.path.join(_HERE, "libbbai_hip.so")      # (override: experiment builds)
ATLAS_PATH = os.path.join(_HERE, "data", "tile_atlas_ts8.npz")
VIEW_ATLAS_PATH = os.path.join(_HERE, "data", "tile_atlas_ts%d.npz")      # the 7x7 view's picture, per tile size (8: tracked; 16 / 32: written by build() with tools/gen_atlas.py --tile-size)
GRID_ATLAS_PATH = os.path.join(_HERE, "data", "grid_atlas_ts%d.npz")      # full-grid picture, per tile size (written by build(): tools/gen_grid_atlas.py)
GRID_TILE_SIZES = (8, 16, 32)

OBS_BYTES = 147
PIX = 56
PROG_BYTES = 112
TOK_MAX = 72

_lib = None


class EngineError(RuntimeError):
    pass


def check_tile_size(tile_size):
    """RGBImgObsWrapper's / RGBImgPartialObsWrapper's tile size, checked before any device work: the engine has atlases for
    GRID_TILE_SIZES only."""
    ts = int(tile_size)
    if ts != tile_size or ts not in GRID_TILE_SIZES:
        raise ValueError("tile_size %r: the engine has atlases for %s only (tools/gen_grid_atlas.py, tools/gen_atlas.py make them)" % (tile_size, GRID_TILE_SIZES))
    return ts


VIEW_SIZES = (3, 5, 7, 9, 11)


def check_view_size(view_size, pixel=False, full_obs=False):
    """ViewSizeWrapper's agent_view_size, checked before any device work: an odd int in VIEW_SIZES; another size than 7 goes with neither
    pixel nor full_obs (the pixel view kernels draw 7x7 views; the full observation has no view)."""
    if isinstance(view_size, (bool, np.bool_)) or not isinstance(view_size, (int, np.integer)) or int(view_size) not in VIEW_SIZES:
        raise ValueError("view_size %r: an odd int in %s" % (view_size, VIEW_SIZES))
    if int(view_size) != 7 and (pixel or full_obs):
        raise ValueError("view_size %d with %s: partial-view pixels and the full observation exist at the 7x7 view only"
                         % (view_size, "pixel=True" if pixel else "full_obs=True"))
    return int(view_size)


P, I64, I32, F64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double
_STEP = [P, P, P, P, P, P, P, I32]      # env, actions, image, direction, reward, reward64, done, auto_reset: how every stepping entry begins

# include/bbai.h as ctypes sees it, in the header's order: entry -> (restype, argtypes).  tests/test_binding_host.py holds every row to its prototype.
ABI = {
    "bbai_version": (I32, []),
    "bbai_last_error": (ctypes.c_char_p, []),
    "bbai_fill_layout": (I32, [P]),
    "bbai_create": (I32, [P, I64, I32, ctypes.POINTER(P)]),
    "bbai_destroy": (None, [P]),
    "bbai_seed": (I32, [P, P, I64]),
    "bbai_reset": (I32, [P, P, P, P]),
    "bbai_step": (I32, _STEP + [P]),
    "bbai_set_atlas": (I32, [P, P, I32, P]),
    "bbai_render": (I32, [P, P, P, P]),
    "bbai_step_render": (I32, _STEP + [P, P]),
    "bbai_set_render_target": (I32, [P, P]),
    "bbai_render_invalidate": (I32, [P]),
    "bbai_render_shadow": (I32, [P, P, P]),
    "bbai_set_grid_atlas": (I32, [P, I32, P, I32, P]),
    "bbai_render_grid": (I32, [P, I32, I32, P, I64, P, P]),
    "bbai_set_view_atlas": (I32, [P, I32, P, I32, P]),
    "bbai_render_view": (I32, [P, I32, P, I64, P, I64, P, P]),
    "bbai_observe_full": (I32, [P, P, I64, P, P]),
    "bbai_step_full": (I32, _STEP + [P, P]),
    "bbai_set_token_buffer": (I32, [P, P]),
    "bbai_export_state": (I32, [P, I64, I64, P, P, P]),
    "bbai_import_state": (I32, [P, I64, I64, P, P, P]),
    "bbai_get_programs": (I32, [P, I64, I64, P]),
    "bbai_save_state": (I32, [P, P, I64, P, P, P, P, P]),
    "bbai_load_state": (I32, [P, P, P, I64, I64, P, P, P, P, P, P, P]),
    "bbai_reseed": (I32, [P, P, P, I64, P, P, P]),
    "bbai_checkpoint_bytes": (I64, [P]),
    "bbai_checkpoint_save": (I32, [P, P, I64]),
    "bbai_checkpoint_load": (I32, [P, P, I64]),
    "bbai_bot_act": (I32, [P, P, P, P]),
    "bbai_bot_rollout": (I32, [P, I32, P, P, P, P, P, P, P, P, P, P]),
    "bbai_bot_stats": (I32, [P, P, P]),
    "bbai_tap": (I32, [I64, I64] + [P] * 11),
    "bbai_tap_ids": (I32, [I64, I64] + [P] * 12),
    "bbai_step_tap_set": (I32, [P, P, I64]),
    "bbai_step_tapped": (I32, _STEP + [P, P, P, P, P]),
    "bbai_rollout": (I32, [P, I32, P, P, P, P, P, P, I32, P, P, P]),
    "bbai_gae": (I32, [I64, I32, P, P, P, P, P, F64, F64, P, P, P]),
    "bbai_demo_spans": (I32, [I64, I32, P, P, P, I64, I32, P, P, P, P, P]),
    "bbai_demo_pack": (I32, [I64, I64, I32] + [P] * 8),
    "bbai_demo_jobs": (I32, [I64, I32, P, P, P, I64, P, P, P, I64, P, P, P, P, P]),
    "bbai_demo_pack_list": (I32, [I64, I64, I64, I32, I32] + [P] * 8),
    "bbai_demo_batch": (I32, [I64, I64] + [P] * 14),
    "bbai_profile": (I32, [P, I32]),
    "bbai_profile_read": (I32, [P, P, P]),
    "bbai_set_call_events": (I32, [P, I32]),
    "bbai_set_done_actions": (I32, [P, I32]),
    "bbai_get_done_actions": (I32, [P]),
    "bbai_set_option": (I32, [P, ctypes.c_char_p, I64]),
    "bbai_get_option": (I32, [P, ctypes.c_char_p, ctypes.POINTER(I64)]),
    "bbai_reset_count": (I32, [P, P]),
    "bbai_generator_failures": (I32, [P, P]),
}
EXPORTED_SYMBOLS = tuple(ABI)

# include/bbai_demo_replay.h, the companion header of the replay entries, the same way (tests/test_demo_replay_abi.py holds the rows to it)
ABI_REPLAY = {
    "bbai_demo_replay_feed": (I32, [I64, P, P, P, P, P, I64, I64] + [P] * 11),
    "bbai_demo_replay_judge": (I32, [I64, P, P, P, P, P, I64, P, P, P, P, I32, P, P, I64, P, P, P, P]),
}
REPLAY_SYMBOLS = tuple(ABI_REPLAY)

# include/bbai_view_size.h, the companion header of the view-size entries, the same way (tests/test_view_size_host.py holds the rows to it)
ABI_VIEW = {
    "bbai_observe_view": (I32, [P, I32, P, I64, P, P]),
    "bbai_step_view": (I32, _STEP + [I32, P, P]),
}
VIEW_SYMBOLS = tuple(ABI_VIEW)

# include/bbai_view_pixels.h, the companion header of the any-view-size pixel entries, the same way (tests/test_view_pixels_host.py holds the rows to it)
ABI_VIEW_PIXELS = {
    "bbai_set_view_pixels_atlas": (I32, [P, I32, P, I32, P]),
    "bbai_render_view_pixels": (I32, [P, I32, I32, P, I64, P, I64, P, P]),
}
VIEW_PIXELS_SYMBOLS = tuple(ABI_VIEW_PIXELS)

# include/bbai_grid_target.h, the companion header of the registered full-grid target, the same way (tests/test_grid_delta_host.py holds the rows to it)
ABI_GRID_TARGET = {
    "bbai_set_grid_target": (I32, [P, P, I32]),
    "bbai_render_grid_target": (I32, [P, P]),
    "bbai_step_grid_target": (I32, _STEP + [P]),
    "bbai_grid_target_invalidate": (I32, [P]),
    "bbai_grid_target_shadow": (I32, [P, P, P]),
}
GRID_TARGET_SYMBOLS = tuple(ABI_GRID_TARGET)

# k_view_pixels_n's launch shape (babyai_amd/csrc/bbai_viewpxn.hpp: VIEWPXN_BLOCK, VIEWPXN_ITEM_BYTES, VIEWPXN_SLICE_MIN, viewpxn_items;
# tests/test_view_pixels_host.py holds view_pixels_items to the header's function)
VIEW_PIXELS_BLOCK = 1024
VIEW_PIXELS_ITEM_BYTES = 150528
VIEW_PIXELS_SLICE_MIN = 65536
VIEW_PIXELS_BLOCKS_PER_CU = 2


def view_pixels_items(view_size, tile_size, count, cus):
    """(envs_per_item, slices, items, blocks) of a bbai_render_view_pixels launch of `count` frames on a device with `cus` compute units:
    work items of at most VIEW_PIXELS_ITEM_BYTES of frames -- whole frames, as many as the block has lanes for their cells, fewer while that
    still leaves an item per block; or slices of one frame where a frame is larger, twice as many for frames of VIEW_PIXELS_SLICE_MIN
    bytes or more while there are fewer items than blocks -- over persistent blocks, VIEW_PIXELS_BLOCKS_PER_CU per compute unit."""
    want = cus * VIEW_PIXELS_BLOCKS_PER_CU
    cells = view_size * view_size
    nbytes = 3 * cells * tile_size * tile_size
    epi, slices = min(VIEW_PIXELS_ITEM_BYTES // nbytes, VIEW_PIXELS_BLOCK // cells), 1
    if epi > 1 and count // want < epi:
        epi = count // want
    epi = max(epi, 1)
    if epi == 1:
        slices = -(-nbytes // VIEW_PIXELS_ITEM_BYTES)
        if nbytes >= VIEW_PIXELS_SLICE_MIN and count * slices < want:
            slices *= 2
    items = count * slices if slices > 1 else -(-count // epi)
    return epi, slices, items, max(1, min(items, want))


def bind(lib):
    """Give every entry of ABI, ABI_REPLAY, ABI_VIEW, ABI_VIEW_PIXELS and ABI_GRID_TARGET that `lib` has its restype and argtypes.  An entry it lacks is passed over (A/B runs against older
    experiment builds, BBAI_ENGINE_LIB: they lack the newer entries; the callers that have a way round ask hasattr(lib, name))."""
    for name, (restype, argtypes) in list(ABI.items()) + list(ABI_REPLAY.items()) + list(ABI_VIEW.items()) + list(ABI_VIEW_PIXELS.items()) + list(ABI_GRID_TARGET.items()):
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return lib


def load_library():
    """dlopen the HIP engine; raises EngineError (never falls back to a CPU path)."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise EngineError("HIP engine %s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
        # torch first: the PyTorch-ROCm wheel carries its own libamdhip64; whichever HIP runtime is mapped first serves
        # the whole process, and the engine must share torch's (device pointers and streams cross the boundary).
        import torch  # noqa: F401
        _lib = bind(ctypes.CDLL(LIB_PATH))
    return _lib


def seeds_u64(seeds, what):
    """uint64[k] on the host from a seed list: a uint64 ndarray as it is, else any sequence or array of integers in [0, 2^64) -- ValueError
    ("negative" / "uint64", after `what`) for a value outside."""
    if isinstance(seeds, np.ndarray) and seeds.dtype == np.uint64:
        return np.ascontiguousarray(seeds).reshape(-1)
    vals = [int(v) for v in np.asarray(seeds if isinstance(seeds, np.ndarray) else list(seeds), dtype=object).reshape(-1)]
    if any(v < 0 for v in vals):
        raise ValueError("%s: negative seed" % what)
    if any(v >= 1 << 64 for v in vals):
        raise ValueError("%s: seeds are uint64" % what)
    return np.array(vals, dtype=np.uint64)


def reseed_levels_arg(levels, what):
    """A `levels=` / `reseed_levels=` argument as None or an int >= 0 -- ValueError (after `what`) for anything that is not an integer (bool
    and float included) and for a negative one."""
    if levels is None:
        return None
    if isinstance(levels, (bool, np.bool_)) or not isinstance(levels, (int, np.integer)):
        raise ValueError("%s: levels must be None or an integer, got %r" % (what, levels))
    if int(levels) < 0:
        raise ValueError("%s: levels must not be negative, got %d" % (what, int(levels)))
    if int(levels) > 0x7fffffff:
        return 0            # (beyond any ring: the whole ring)
    return int(levels)


def load_atlas(path, tool):
    """(tiles, lut) of a tile atlas file as contiguous uint8; `tool`: what writes the file, for the EngineError if it is not there."""
    if not os.path.isfile(path):
        raise EngineError("tile atlas %s not built: run `python -c 'import __graft_entry__ as g; g.build()'` (%s)" % (path, tool))
    with np.load(path) as f:
        return np.ascontiguousarray(f["tiles"], dtype=np.uint8), np.ascontiguousarray(f["lut"], dtype=np.uint8)


def _check(lib, rc, what):
    if rc != 0:
        raise EngineError("%s failed (%d): %s" % (what, rc, lib.bbai_last_error().decode()))


class TapLog(ctypes.Structure):
    """include/bbai.h bbai_tap_log"""
    _fields_ = [("count", ctypes.c_int64), ("pix_count", ctypes.c_int64), ("ids_dev", ctypes.c_void_p), ("image_out", ctypes.c_void_p),
                ("dir_out", ctypes.c_void_p), ("reward64_out", ctypes.c_void_p), ("done_out", ctypes.c_void_p), ("pixels_out", ctypes.c_void_p),
                ("obs_row0", ctypes.c_int64), ("row0", ctypes.c_int64)]


class Missions(object):
    """Lazy per-env mission strings: compiled programs are fetched from HBM and rendered to
    text only when a consumer indexes them."""

    def __init__(self, env):
        self._env = env
        self._progs = None
        self._cache = {}
        self._version = env._obs_version          # the step / reset this view belongs to

    def _fetch(self):
        if self._progs is None:
            if self._version != self._env._obs_version:
                # the programs in HBM have moved on (an auto-reset may have replaced this env's mission): refuse to hand
                # out the NEXT episode's text for an observation of an earlier step
                raise EngineError("mission view of an earlier step: index obs['mission'] before the next step()/reset(), "
                                  "or take env.missions() when the observation is produced")
            self._progs = self._env.programs()
        return self._progs

    def snapshot(self):
        """Fetch the programs NOW (n x 112 bytes to the host): the view stays valid after later steps.  The list-of-dicts
        adapters do this for every observation they hand out (the reference's collectors read missions of stored
        observations many steps later, babyai/rl/algos/base.py:207-232)."""
        self._fetch()
        return self

    def __len__(self):
        return self._env.num_envs

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        i = int(i)
        if i < 0:
            i += len(self)
        s = self._cache.get(i)
        if s is None:
            s = missions.prog_surface(self._fetch()[i])
            self._cache[i] = s
        return s

    def __iter__(self):
        return (self[i] for i in range(len(self)))



class EnvSnapshot(object):
    """The live state of R envs as four tensors (include/bbai.h bbai_save_state): `rec` uint8[R, rec_bytes], `hot` uint8[R, 16], `stale`
    int64[R] (the uint64 stale sets' bits), `lsm` uint8[R] (lastStepMatch bytes: done-action mode; zeros otherwise) -- rows as
    export_state() returns them -- plus the level, record size and verifier mode they belong to.  Valid in any batch of the same level,
    `rec_bytes` and done-action mode, whatever its size, state layout or look-ahead depth.  Holds no look-ahead levels, no RNG stream and no
    expert plan.  select / cat / to are torch ops and work on CPU tensors too (a replay buffer of levels may live on the host)."""

    def __init__(self, rec, hot, stale, lsm, env_id, rec_bytes, done_actions):
        self.rec, self.hot, self.stale, self.lsm = rec, hot, stale, lsm
        self.env_id, self.rec_bytes, self.done_actions = level_name(env_id), int(rec_bytes), bool(done_actions)
        r = int(rec.shape[0])
        if tuple(rec.shape) != (r, self.rec_bytes) or tuple(hot.shape) != (r, 16) or tuple(stale.shape) != (r,) or tuple(lsm.shape) != (r,):
            raise ValueError("snapshot tensors: rec [R, %d], hot [R, 16], stale [R], lsm [R]" % self.rec_bytes)

    def __len__(self):
        return int(self.rec.shape[0])

    @property
    def device(self):
        return self.rec.device

    def _like(self, rec, hot, stale, lsm):
        return EnvSnapshot(rec, hot, stale, lsm, self.env_id, self.rec_bytes, self.done_actions)

    def select(self, rows):
        """The snapshot of rows `rows` (an int sequence or an int64 tensor on the snapshot's device; any order, repeats allowed)."""
        import torch
        if not isinstance(rows, torch.Tensor):
            rows = torch.as_tensor(np.asarray(rows, dtype=np.int64).reshape(-1), device=self.rec.device)
        return self._like(self.rec[rows].contiguous(), self.hot[rows].contiguous(), self.stale[rows].contiguous(), self.lsm[rows].contiguous())

    @staticmethod
    def cat(snaps):
        """One snapshot of the rows of several (same level, record size and done-action mode; same device)."""
        import torch
        snaps = list(snaps)
        if not snaps:
            raise ValueError("EnvSnapshot.cat of nothing")
        a = snaps[0]
        for b in snaps[1:]:
            if (b.env_id, b.rec_bytes, b.done_actions) != (a.env_id, a.rec_bytes, a.done_actions):
                raise ValueError("EnvSnapshot.cat: snapshots of %s (rec_bytes %d, done_actions %s) and %s (rec_bytes %d, done_actions %s)"
                                 % (a.env_id, a.rec_bytes, a.done_actions, b.env_id, b.rec_bytes, b.done_actions))
        return a._like(*(torch.cat([getattr(x, k) for x in snaps]) for k in ("rec", "hot", "stale", "lsm")))

    def to(self, device):
        return self._like(self.rec.to(device), self.hot.to(device), self.stale.to(device), self.lsm.to(device))


class BatchedBabyAIEnv(object):
    """N environments of one BabyAI level on one MI355X.

    Parameters
    ----------
    env_id : 'BabyAI-<Level>-v0' or '<Level>' (babyai/levels/levelgen.py:480)
    num_envs : number of parallel envs on this device
    device : torch device string / index (a ROCm GPU)
    pixel : apply RGBImgPartialObsWrapper semantics (obs image uint8[N, 7*tile_size, 7*tile_size, 3]: [N,56,56,3] at the default 8)
    auto_reset : True = ParallelEnv protocol (penv.py:8-11); False = ManyEnvs protocol
                 (evaluate.py:73-81: finished envs freeze until reset())
    done_actions : the reference's BABYAI_DONE_ACTIONS verifier mode (babyai/levels/verifier.py:17,216-230: an instruction
                 succeeds only on a `done` action right after the step that completed it; include/bbai.h
                 bbai_set_done_actions).  None (default) = as the reference decides it: on iff that environment variable is
                 non-empty; True / False force it for this batch
    full_obs : the fully observable wrappers instead of the 7x7 view: obs image = FullyObsWrapper's uint8[N, W, H, 3] (`full`; pixel=False)
                 or RGBImgObsWrapper's uint8[N, H*tile_size, W*tile_size, 3] (pixel=True: render('rgb_array', highlight=False)); the
                 obs dict then has no use for 'direction', which the list-of-dicts adapters leave out as the wrappers do.  The 7x7
                 `image`, `direction`, rewards and dones are computed and kept as without it
    tile_size : the pixel wrappers' tile size, 8, 16 or 32 (anything else with pixel=True: ValueError) -- RGBImgObsWrapper's with
                 full_obs=True, RGBImgPartialObsWrapper's without.  With full_obs=True `full` is registered as the handle's full-grid target
                 (include/bbai_grid_target.h): reset(), step(), load_state(), reseed() and rollout() store only the 64-byte pieces of a frame
                 that changed -- a turn changes one cell, a move two, only a reset the whole grid (set_option("grid_render_delta", 0) draws
                 every frame whole again; after writing into `full` yourself call render_invalidate()).  The partial view at 8 is the 56x56 path with its delta render
                 (9.4 KB per env per frame); at 16 / 32 `pixels` is uint8[N,112,112,3] / [N,224,224,3], 37.6 KB / 150.5 KB per env --
                 65 536 envs at 32 are 9.9 GB -- and is registered as the handle's render target of that size: reset(), step(),
                 load_state() and reseed() store only the 64-byte pieces of a frame that changed (include/bbai.h bbai_render_view,
                 option "render_target_tile_size"; set_option("render_delta", 0) draws every frame whole again; after writing into
                 `pixels` yourself call render_invalidate())
    view_size : ViewSizeWrapper(env, view_size): the egocentric view at 3, 5, 9 or 11 cells instead of 7 -- obs image = uint8[N, V, V, 3]
                 (`view`; include/bbai_view_size.h bbai_observe_view / bbai_step_view), the agent at view cell (V // 2, V - 1).  `image` stays the 7x7
                 encoding and direction, rewards and dones are what they are without it.  Only with pixel=False and full_obs=False, and
                 anything but an odd int in 3..11 is a ValueError; the device expert (bot_actions, bot_rollout) sees 7x7 whatever is
                 observed, so those calls raise on such a batch
    validate_actions : check every step()'s actions on the device first and raise AssertionError("unknown action") like
                 the reference (gym_minigrid MiniGridEnv.step) instead of treating bytes 8..255 as `done` (include/bbai.h);
                 costs one reduction and a host synchronisation per step, so it is off by default
    """

    view_size, view = 7, None          # (class defaults: a batch is the 7x7 one until __init__ says otherwise)
    _grid_target = False               # (... and has no registered full-grid target)

    def __init__(self, env_id, num_envs, device="cuda:0", seeds=None, pixel=False, auto_reset=True, validate_actions=False,
                 done_actions=None, full_obs=False, tile_size=8, view_size=7):
        import torch
        self.torch = torch
        self.full_obs = bool(full_obs)
        self.view_size = check_view_size(view_size, pixel, full_obs)
        self.tile_size = check_tile_size(tile_size) if pixel else int(tile_size)
        if not torch.cuda.is_available():
            raise EngineError("no ROCm GPU visible: the batched engine has no CPU path")
        self.lib = load_library()
        self.env_id = env_id
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise EngineError("device must be a ROCm GPU, got %r" % (device,))
        self.dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.pixel = bool(pixel)
        self.auto_reset = bool(auto_reset)
        self.validate_actions = bool(validate_actions)
        self.cfg = make_cfg(env_id)
        self.handle = ctypes.c_void_p()
        _check(self.lib, self.lib.bbai_create(ctypes.byref(self.cfg), self.num_envs, self.dev_index,
                                               ctypes.byref(self.handle)), "bbai_create")
        if done_actions is not None:
            _check(self.lib, self.lib.bbai_set_done_actions(self.handle, 1 if done_actions else 0), "bbai_set_done_actions")
        self.done_actions = bool(self.lib.bbai_get_done_actions(self.handle))
        self._missions = None
        self._obs_version = 0
        self._atlases = set()          # (picture, tile size) of the tile atlases installed on the handle (_install_atlas)
        self._hold = {}                # entry -> the tensors its last call handed to the device: alive until that entry's next call
        self.instr = None              # enable_instr_tokens(): uint8[N, 72]
        self._bot_out = None           # bot_actions(): its default output
        self._step_tap = 0             # set_step_tap(): how many envs step_tapped() logs
        n = self.num_envs
        with torch.cuda.device(self.dev_index):
            self.image = torch.zeros((n, 7, 7, 3), dtype=torch.uint8, device=self.device)
            self.direction = torch.zeros((n,), dtype=torch.uint8, device=self.device)
            self.reward = torch.zeros((n,), dtype=torch.float32, device=self.device)
            # the reference's own return value: a Python float = float64 (levelgen.py:59-61); `reward` is its f32 rounding
            self.reward64 = torch.zeros((n,), dtype=torch.float64, device=self.device)
            self.done = torch.zeros((n,), dtype=torch.uint8, device=self.device)
            self.pixels = None
            self.full = None        # full_obs: the observation image (observe_full)
            self.view = None        # view_size != 7: the observation image (observe_view)
            if self.view_size != 7:
                self.view = torch.zeros((n, self.view_size, self.view_size, 3), dtype=torch.uint8, device=self.device)
            if self.full_obs:
                c, ts = self.cfg, self.tile_size
                shape = (n, c.H * ts, c.W * ts, 3) if self.pixel else (n, c.W, c.H, 3)
                self.full = torch.zeros(shape, dtype=torch.uint8, device=self.device)
                if self.pixel and all(hasattr(self.lib, name) for name in GRID_TARGET_SYMBOLS):
                    # RGBImgObsWrapper(env, ts): self.full is registered as the handle's full-grid target -- reset(), step(), load_state(), reseed()
                    # and rollout() store only the 64-byte pieces of a frame that changed (include/bbai_grid_target.h; a library without the
                    # entries draws every frame whole with bbai_render_grid)
                    self._install_atlas("grid", ts)
                    _check(self.lib, self.lib.bbai_set_grid_target(self.handle, self.full.data_ptr(), ts), "bbai_set_grid_target")
                    self._grid_target = True
            elif self.pixel:
                # RGBImgPartialObsWrapper(env, ts): frames by bbai_render at 8, by bbai_render_view at 16 / 32.  self.pixels is registered as
                # the handle's target of that tile size: whole-batch renders into it store only the pieces that changed (include/bbai.h
                # bbai_set_render_target, option "render_target_tile_size"; a library without the entry -- at 16 / 32: without the option --
                # draws whole frames)
                ts = self.tile_size
                self.pixels = torch.zeros((n, 7 * ts, 7 * ts, 3), dtype=torch.uint8, device=self.device)
                self._install_atlas("view", ts)
                if hasattr(self.lib, "bbai_set_render_target") and (ts == 8 or self._has_option("render_target_tile_size")):
                    if ts != 8:
                        self.set_option("render_target_tile_size", ts)
                    _check(self.lib, self.lib.bbai_set_render_target(self.handle, self.pixels.data_ptr()), "bbai_set_render_target")
        # (the five output tensors are never replaced: their pointers are taken once, see _step_out)
        self._out_ptrs = tuple(t.data_ptr() for t in (self.image, self.direction, self.reward, self.reward64, self.done))
        self.kernel_events = None      # bench.py: list of (tag, start_event, end_event) when enabled
        self.num_actions = 7
        self.max_mission_tokens = min(TOK_MAX, missions.max_mission_tokens(self.cfg))
        self.max_steps_bound = 8 * self.cfg.room_size ** 2 * self.cfg.num_rows * self.cfg.num_cols
        if seeds is not None:
            self.seed(seeds)

    # ---- protocol ---------------------------------------------------------------------
    def seed(self, seeds):
        """env.seed(s) for every env: an int base (env i gets base + i) or a sequence."""
        if isinstance(seeds, (int, np.integer)):
            seeds = np.arange(self.num_envs, dtype=np.uint64) + np.uint64(seeds)
        seeds = seeds_u64(seeds, "seed")
        if seeds.shape != (self.num_envs,):
            raise ValueError("need %d seeds, got shape %s" % (self.num_envs, seeds.shape))
        _check(self.lib, self.lib.bbai_seed(self.handle, seeds.ctypes.data, self.num_envs), "bbai_seed")
        self.seeds = seeds
        return list(int(s) for s in seeds[:8])

    def _ev_begin(self):
        if self.kernel_events is None:
            return None
        ev = self.torch.cuda.Event(enable_timing=True)
        ev.record(self.torch.cuda.current_stream(self.dev_index))   # same stream the kernels launch on
        return ev

    def _ev_end(self, tag, start):
        if start is None:
            return
        end = self.torch.cuda.Event(enable_timing=True)
        end.record(self.torch.cuda.current_stream(self.dev_index))
        self.kernel_events.append((tag, start, end))

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.dev_index).cuda_stream)

    def _obs(self, rendered=False):
        img = self.image
        if self.full_obs:
            if not rendered:
                ev = self._ev_begin()
                self.observe_full()
                self._ev_end("full_obs", ev)
            img = self.full
        elif self.view is not None:
            if not rendered:
                ev = self._ev_begin()
                self.observe_view()
                self._ev_end("view_obs", ev)
            img = self.view
        elif self.pixel and rendered:
            img = self.pixels
        elif self.pixel:
            ev = self._ev_begin()
            img = self._render_batch_into(self.image, self.tile_size, self.pixels)
            self._ev_end("render", ev)
        return self._obs_dict(img)

    def _moved_on(self):
        """Behind every call that steps or replaces envs: the mission views handed out so far belong to an earlier step (Missions._fetch)."""
        self._obs_version += 1

    def _obs_dict(self, img):
        """The observation dict of the step, reset or load that was just enqueued, with its own mission view."""
        self._moved_on()
        self._missions = Missions(self)
        return {"image": img, "direction": self.direction, "mission": self._missions}

    def _step_out(self):
        """What every stepping entry takes behind its actions (include/bbai.h bbai_step): image, direction, reward, reward64, done, auto_reset."""
        return self._out_ptrs + (1 if self.auto_reset else 0,)

    def render_encoding(self, image=None, out=None, tile_size=None, view_size=None):
        """RGBImgPartialObsWrapper(env, tile_size).observation for ANY encoded batch uint8[N,7,7,3] on the device (default: the current
        one) -> uint8[N,7ts,7ts,3], at the batch's tile size or the one given (include/bbai.h bbai_render at 8 -> [N,56,56,3];
        bbai_render_view at 16 / 32, any number of rows, `out` allocated when there is none of that shape).  step() / reset() already
        return pixels in pixel mode; this is for stored or hand-made encodings.
        view_size=V other than 7: the picture RGBImgPartialObsWrapper(ViewSizeWrapper(env, V), tile_size) draws of a contiguous
        uint8[k, V, V, 3] encoding on the device (observe_view's frames, stored ones) -> uint8[k, V ts, V ts, 3]
        (include/bbai_view_pixels.h bbai_render_view_pixels; `out` allocated when none is given; tile_size None = the batch's)."""
        if view_size is not None and check_view_size(view_size) != 7:
            v = int(view_size)
            ts = check_tile_size(self.tile_size if tile_size is None else tile_size)
            torch = self.torch
            if image is None or image.dtype != torch.uint8 or image.device != self.device or not image.is_contiguous() or \
                    image.dim() != 4 or tuple(image.shape[1:]) != (v, v, 3):
                raise ValueError("image: contiguous uint8[k, %d, %d, 3] on %s" % (v, v, self.device))
            k = int(image.shape[0])
            out = self._frames_out(out, (k, v * ts, v * ts, 3))
            return self._view_pixels_into(image, None, k, v, ts, out)
        image = self.image if image is None else image
        ts = self.tile_size if tile_size is None and self.pixel and not self.full_obs else 8 if tile_size is None else check_tile_size(tile_size)
        if ts != 8:
            torch = self.torch
            if image.dtype != torch.uint8 or image.device != self.device or not image.is_contiguous() or image.numel() % OBS_BYTES:
                raise ValueError("image: contiguous uint8[k, 7, 7, 3] on %s" % (self.device,))
            k = image.numel() // OBS_BYTES
            if out is None and self.pixels is not None and tuple(self.pixels.shape) == (k, 7 * ts, 7 * ts, 3):
                out = self.pixels
            out = self._frames_out(out, (k, 7 * ts, 7 * ts, 3))
            return self._render_view_into(image, None, k, ts, out)
        return self._render_batch_into(image, 8, self.pixels if out is None else out)

    def _install_atlas(self, picture, ts):
        """The tile atlas of `picture` at tile size ts on the handle, on first use: "view" = the agent's 7x7 view (8: bbai_render's 56x56 atlas;
        16 / 32: bbai_render_view's), "grid" = the full grid (bbai_render_grid), "view_pixels" = the view at any view size
        (bbai_render_view_pixels)."""
        if (picture, ts) in self._atlases:
            return
        if picture == "grid":
            tiles, lut = load_atlas(GRID_ATLAS_PATH % ts, "tools/gen_grid_atlas.py")
            _check(self.lib, self.lib.bbai_set_grid_atlas(self.handle, ts, tiles.ctypes.data, tiles.shape[0], lut.ctypes.data), "bbai_set_grid_atlas")
        elif picture == "view_pixels":      # (the view's atlas files once more, for bbai_render_view_pixels: the handle keeps them apart)
            if not all(hasattr(self.lib, name) for name in VIEW_PIXELS_SYMBOLS):
                raise EngineError("this engine library has no %s (pixels at view_size other than 7)" % " / ".join(VIEW_PIXELS_SYMBOLS))
            tiles, lut = load_atlas(VIEW_ATLAS_PATH % ts, "tools/gen_atlas.py" + (" --tile-size %d" % ts if ts != 8 else ""))
            _check(self.lib, self.lib.bbai_set_view_pixels_atlas(self.handle, ts, tiles.ctypes.data, tiles.shape[0], lut.ctypes.data), "bbai_set_view_pixels_atlas")
        elif ts == 8:
            tiles, lut = load_atlas(ATLAS_PATH, "tools/gen_atlas.py")
            _check(self.lib, self.lib.bbai_set_atlas(self.handle, tiles.ctypes.data, tiles.shape[0], lut.ctypes.data), "bbai_set_atlas")
        else:
            if not hasattr(self.lib, "bbai_render_view"):
                raise EngineError("this engine library has no bbai_render_view (tile_size %d)" % ts)
            tiles, lut = load_atlas(VIEW_ATLAS_PATH % ts, "tools/gen_atlas.py --tile-size %d" % ts)
            _check(self.lib, self.lib.bbai_set_view_atlas(self.handle, ts, tiles.ctypes.data, tiles.shape[0], lut.ctypes.data), "bbai_set_view_atlas")
        self._atlases.add((picture, ts))

    def _render_view_into(self, image, ids_ptr, k, ts, out):
        """bbai_render_view: rows `ids_ptr` (None = the first k) of the encoded buffer `image` -> out uint8[k, 7ts, 7ts, 3]."""
        self._install_atlas("view", ts)
        _check(self.lib, self.lib.bbai_render_view(self.handle, ts, image.data_ptr(), image.numel() // OBS_BYTES, ids_ptr, k,
                                                    out.data_ptr() if k else None, self._stream()), "bbai_render_view")
        return out

    def _render_batch_into(self, image, ts, out):
        """num_envs encoded rows -> num_envs frames of tile size ts: bbai_render at 8, bbai_render_view at 16 / 32."""
        if ts != 8:
            return self._render_view_into(image, None, self.num_envs, ts, out)
        _check(self.lib, self.lib.bbai_render(self.handle, image.data_ptr(), out.data_ptr(), self._stream()), "bbai_render")
        return out

    def _view_pixels_into(self, image, ids_ptr, k, v, ts, out):
        """bbai_render_view_pixels: rows `ids_ptr` (None = the first k) of the encoded buffer `image` uint8[rows, v, v, 3] -> out uint8[k, v ts, v ts, 3]."""
        self._install_atlas("view_pixels", ts)
        _check(self.lib, self.lib.bbai_render_view_pixels(self.handle, v, ts, image.data_ptr() if image.numel() else None, image.numel() // (3 * v * v),
                                                           ids_ptr, k, out.data_ptr() if k else None, self._stream()), "bbai_render_view_pixels")
        return out

    def render_view(self, ids=None, tile_size=None, out=None, view_size=None):
        """The agent's view of envs `ids` (None = every env; else an int sequence or an int64 device tensor, any order, repeats allowed) as
        RGBImgPartialObsWrapper(env, tile_size) draws it, from the current `self.image` -> uint8[k, 7ts, 7ts, 3] on the device,
        asynchronous on the current stream (include/bbai.h bbai_render_view; tile_size None = the batch's).  Available on any batch, also
        an encoded one; the atlas of a tile size is installed on first use.  Writes nothing but `out` (37.6 KB a frame at 16, 150.5 KB
        at 32); an id outside [0, num_envs) gives an all-zero frame.  tile_size=8 goes through bbai_render (56x56 frames).
        view_size=None is exactly that, the 7x7 view from `self.image`, on a view_size batch too.  view_size=V in VIEW_SIZES draws what
        RGBImgPartialObsWrapper(ViewSizeWrapper(env, V), tile_size) shows -> uint8[k, V ts, V ts, 3] (include/bbai_view_pixels.h
        bbai_render_view_pixels): for V other than 7 from the current STATE, on any batch -- observe_view(ids, V) into a scratch encoding,
        or `self.view` as it stands for every env of a view_size=V batch -- and for an explicit 7 from `self.image`, which at tile size
        8 draws the listed envs in one native launch where the default call gathers rows and pads runs for bbai_render."""
        torch = self.torch
        ts = check_tile_size(self.tile_size if tile_size is None else tile_size)
        if view_size is not None:
            v = check_view_size(view_size)
            k, ids_ptr, ids_t = self._ids(ids)
            out = self._frames_out(out, (k, v * ts, v * ts, 3))
            if v == 7:
                self._hold["render_view"] = ids_t
                return self._view_pixels_into(self.image, ids_ptr, k, 7, ts, out)
            if self.view is not None and ids is None and v == self.view_size:
                self._hold["render_view"] = None
                return self._view_pixels_into(self.view, None, k, v, ts, out)
            # the listed envs' V x V encodings from the state, row j = ids[j] (an id outside the batch: a zero row, drawn as the
            # unseen tile -- so such frames are zeroed by listing their rows as outside the scratch buffer)
            enc = self.observe_view(ids_t, v)
            rows_ptr, rows_t = None, None
            if ids_t is not None:
                with torch.cuda.device(self.dev_index):
                    rows_t = torch.arange(k, dtype=torch.int64, device=self.device)
                    rows_t = torch.where((ids_t < 0) | (ids_t >= self.num_envs), torch.full_like(rows_t, -1), rows_t)
                rows_ptr = rows_t.data_ptr()
            self._hold["render_view"] = (ids_t, enc, rows_t)
            return self._view_pixels_into(enc, rows_ptr, k, v, ts, out)
        k, ids_ptr, ids_t = self._ids(ids)
        out = self._frames_out(out, (k, 7 * ts, 7 * ts, 3))
        if ts != 8:
            self._hold["render_view"] = ids_t
            return self._render_view_into(self.image, ids_ptr, k, ts, out)
        if k == 0:
            return out
        # bbai_render draws num_envs rows into num_envs frames: the listed rows are gathered and go through in runs of num_envs
        self._install_atlas("view", 8)
        n = self.num_envs
        with torch.cuda.device(self.dev_index):
            enc, bad = self.image, None
            if ids_t is not None:
                bad = (ids_t < 0) | (ids_t >= n)
                enc = self.image[ids_t.clamp(0, n - 1)]
            keep = []
            for lo in range(0, k, n):
                m = min(n, k - lo)
                src, dst = enc[lo:lo + m], out[lo:lo + m]
                if m < n:          # a short run: padded on both sides
                    src = torch.cat([src, torch.zeros((n - m, 7, 7, 3), dtype=torch.uint8, device=self.device)])
                    dst = torch.empty((n, PIX, PIX, 3), dtype=torch.uint8, device=self.device)
                _check(self.lib, self.lib.bbai_render(self.handle, src.data_ptr(), dst.data_ptr(), self._stream()), "bbai_render")
                if m < n:
                    out[lo:lo + m] = dst[:m]
                keep.append((src, dst))
            self._hold["render_view"] = (ids_t, keep)
            if bad is not None:
                out[bad] = 0           # an id outside the batch: an all-zero frame, as at 16 / 32
        return out

    def render_grid(self, ids=None, tile_size=32, highlight=True, out=None):
        """MiniGridEnv.render('rgb_array', highlight=highlight, tile_size=tile_size) of envs `ids` (None = every env; else an int sequence or
        an int64 device tensor, any order, repeats allowed) -> uint8[k, H*ts, W*ts, 3] on the device, asynchronous on the current stream
        (include/bbai.h bbai_render_grid).  Reads the current state and writes nothing but `out`; an id outside [0, num_envs) gives an
        all-zero frame.  The atlas of a tile size is installed on first use."""
        ts = check_tile_size(tile_size)
        self._install_atlas("grid", ts)
        k, ids_ptr, self._hold["render_grid"] = self._ids(ids)
        out = self._frames_out(out, (k, self.cfg.H * ts, self.cfg.W * ts, 3))
        _check(self.lib, self.lib.bbai_render_grid(self.handle, ts, 1 if highlight else 0, ids_ptr, k, out.data_ptr() if k else None,
                                                    self._stream()), "bbai_render_grid")
        return out

    def _ids(self, ids):
        """An env id list -- None = every env; an int sequence, an ndarray or an int64 device tensor -- as (k, device pointer, int64[k] tensor
        on the device), pointer and tensor None for every env.  The caller keeps the tensor in self._hold until its launch is consumed."""
        torch = self.torch
        if ids is None:
            return self.num_envs, None, None
        if not isinstance(ids, torch.Tensor):
            ids = torch.as_tensor(np.asarray(ids, dtype=np.int64).reshape(-1), device=self.device)
        if ids.dtype != torch.int64 or ids.device != self.device or ids.dim() != 1:
            raise ValueError("ids: int64[k] on %s" % (self.device,))
        ids = ids.contiguous()
        return int(ids.shape[0]), ids.data_ptr(), ids

    def _no_env_twice(self, what, ids, padding=False):
        """ValueError if a HOST-side id list names an env twice (a device list is not read back: there it is undefined which entry wins).
        padding=True: ids outside [0, num_envs) name no env and may repeat (reseed)."""
        if ids is None or isinstance(ids, self.torch.Tensor):
            return
        host = np.asarray(ids, dtype=np.int64).reshape(-1)
        if padding:
            host = host[(host >= 0) & (host < self.num_envs)]
        if len(np.unique(host)) != len(host):
            raise ValueError("%s: an env is listed twice" % what)

    def _frames_out(self, out, shape):
        torch = self.torch
        if out is None:
            with torch.cuda.device(self.dev_index):
                out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous():
            raise ValueError("out: contiguous uint8%s on %s" % (list(shape), self.device))
        return out

    def observe_full(self, ids=None, out=None):
        """The full observation of envs `ids` (None = every env; else an int sequence or an int64 device tensor, any order, repeats
        allowed) from the current state, asynchronous on the current stream: FullyObsWrapper's uint8[k, W, H, 3] (include/bbai.h
        bbai_observe_full) -- or, in a full_obs pixel batch, RGBImgObsWrapper's uint8[k, H*ts, W*ts, 3] (render_grid(ids, tile_size,
        highlight=False)).  ids = out = None in a full_obs batch refreshes `full`, the observation step() returns (after load_checkpoint
        or import_state, which do not carry it).  An id outside [0, num_envs) gives an all-zero frame.  In a full_obs pixel batch `full`
        is the handle's registered full-grid target: refreshing it (ids None, out None or `full`) stores only the 64-byte pieces that
        changed since the frame it holds (include/bbai_grid_target.h bbai_render_grid_target); every other (ids, out) draws whole frames,
        and where `out` lies in `full`'s storage the target's history is dropped."""
        if self.full_obs and ids is None and out is None:
            out = self.full
        if self._grid_target and ids is None and out is self.full:
            _check(self.lib, self.lib.bbai_render_grid_target(self.handle, self._stream()), "bbai_render_grid_target")
            return out
        if self.full_obs and self.pixel:
            return self.render_grid(ids, tile_size=self.tile_size, highlight=False, out=out)
        k, ids_ptr, self._hold["observe_full"] = self._ids(ids)
        out = self._frames_out(out, (k, self.cfg.W, self.cfg.H, 3))
        _check(self.lib, self.lib.bbai_observe_full(self.handle, ids_ptr, k, out.data_ptr() if k else None, self._stream()),
               "bbai_observe_full")
        return out

    def observe_view(self, ids=None, view_size=None, out=None):
        """ViewSizeWrapper(env, view_size)'s observation image of envs `ids` (None = every env; else an int sequence or an int64 device
        tensor, any order, repeats allowed) from the current state -> uint8[k, V, V, 3] on the device, asynchronous on the current stream
        (include/bbai_view_size.h bbai_observe_view; view_size None = the batch's; any of VIEW_SIZES on any batch).  ids = out = None at the batch's
        own size in a view_size batch refreshes `view`, the observation step() returns (after load_checkpoint or import_state, which do
        not carry it).  An id outside [0, num_envs) gives an all-zero frame."""
        v = self.view_size if view_size is None else check_view_size(view_size)
        if self.view is not None and ids is None and out is None and v == self.view_size:
            out = self.view
        k, ids_ptr, self._hold["observe_view"] = self._ids(ids)
        out = self._frames_out(out, (k, v, v, 3))
        _check(self.lib, self.lib.bbai_observe_view(self.handle, v, ids_ptr, k, out.data_ptr() if k else None, self._stream()),
               "bbai_observe_view")
        return out

    def _expert_sees_7x7(self, what):
        """The device expert keeps a 7x7 visibility mask; the reference's bot would use the env's agent_view_size (babyai/bot.py:663-674)."""
        if self.view_size != 7:
            raise EngineError("%s on a view_size=%d batch: the device expert sees 7x7 and would diverge from the reference's bot" % (what, self.view_size))

    def render_invalidate(self):
        """Call after writing into self.pixels -- or, in a full_obs pixel batch, into self.full -- yourself: the next render rewrites every byte
        (include/bbai.h bbai_render_invalidate, include/bbai_grid_target.h bbai_grid_target_invalidate)."""
        _check(self.lib, self.lib.bbai_render_invalidate(self.handle), "bbai_render_invalidate")
        if hasattr(self.lib, "bbai_grid_target_invalidate"):
            _check(self.lib, self.lib.bbai_grid_target_invalidate(self.handle), "bbai_grid_target_invalidate")

    def grid_shadow(self):
        """The tile ids of the frames the registered full-grid target holds, uint8[N][W*H], row-major y*W + x, in the grid atlas of its tile
        size (include/bbai_grid_target.h bbai_grid_target_shadow)."""
        import torch
        out = torch.empty((self.num_envs, self.cfg.W * self.cfg.H), dtype=torch.uint8, device=self.device)
        _check(self.lib, self.lib.bbai_grid_target_shadow(self.handle, out.data_ptr(), self._stream()), "bbai_grid_target_shadow")
        return out

    def render_shadow(self):
        """The tile ids of the frame the registered buffer holds, uint8[N][49] (include/bbai.h bbai_render_shadow)."""
        import torch
        out = torch.empty((self.num_envs, 49), dtype=torch.uint8, device=self.device)      # (a target a caller registered itself: there may be no self.pixels)
        _check(self.lib, self.lib.bbai_render_shadow(self.handle, out.data_ptr(), self._stream()), "bbai_render_shadow")
        return out

    def reset(self):
        _check(self.lib, self.lib.bbai_reset(self.handle, self.image.data_ptr(), self.direction.data_ptr(),
                                              self._stream()), "bbai_reset")
        return self._obs()

    def _step_actions(self, actions, validate, count, hold_ok):
        """step()'s actions as a contiguous uint8[count] tensor on the device.  Host data is checked for free and a device tensor under
        validate / validate_actions: AssertionError("unknown action") beyond RESET_ENV -- beyond HOLD where a hold means something
        (`hold_ok`: True, or None = ask the handle's option "step_hold", and only when an 8 turns up)."""
        torch = self.torch

        def limit(hi):
            ok = hold_ok if hold_ok is not None or hi != self.HOLD else bool(self.get_option("step_hold"))
            return self.HOLD if ok else self.RESET_ENV

        if not isinstance(actions, torch.Tensor):
            actions = np.asarray(actions)
            if actions.size:                                  # host data: checked for free
                lo, hi = int(actions.min()), int(actions.max())
                if lo < 0 or hi > limit(hi):
                    raise AssertionError("unknown action")
            else:
                actions = actions.astype(np.uint8)            # (an empty list has no integer type of its own)
            actions = torch.as_tensor(actions, device=self.device)
        elif self.validate_actions if validate is None else validate:
            # MiniGridEnv.step: `assert False, "unknown action"` (7 = RESET_ENV is this engine's per-env reset command, 8 = HOLD where it is on)
            lo, hi = (int(v) for v in torch.stack([actions.min(), actions.max()]).tolist())
            if lo < 0 or hi > limit(hi):
                raise AssertionError("unknown action")
        if actions.dtype != torch.uint8:
            # a wider integer must not WRAP into a valid action on its way to a byte (263 -> 7 = RESET_ENV, 256 -> 0 = left):
            # everything outside 0..255 becomes 255, which include/bbai.h defines -- like every unknown action -- as `done`
            if actions.dtype.is_floating_point or actions.dtype == torch.bool:
                raise TypeError("actions must be an integer tensor, got %s" % actions.dtype)
            # (ONE extra elementwise launch, then the cast: RL callers step with int64 samples on 30-us steps)
            if actions.dtype == torch.int8:
                actions = actions.to(torch.int16)
            actions = torch.where((actions & -256) != 0, 255, actions)
        if actions.dtype != torch.uint8 or actions.device != self.device or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.uint8).contiguous()
        if actions.numel() != count:
            raise ValueError("need %d actions" % count)
        return actions.reshape(-1)

    def _step_native(self, actions):
        """One step of the whole batch with `actions` uint8[num_envs] on the device: the entry this batch's observation mode steps through."""
        ev = self._ev_begin()
        if self.full_obs and not self.pixel and self.kernel_events is None:
            # FullyObsWrapper's step: transition + the full observation of every env as ONE call (include/bbai.h bbai_step_full)
            _check(self.lib, self.lib.bbai_step_full(self.handle, actions.data_ptr(), *self._step_out(), self.full.data_ptr(), self._stream()),
                   "bbai_step_full")
            return self._obs(rendered=True), self.reward, self.done, {}
        if self._grid_target and self.kernel_events is None:
            # RGBImgObsWrapper's step: transition + the changed pieces of every env's frame as ONE call (include/bbai_grid_target.h bbai_step_grid_target)
            _check(self.lib, self.lib.bbai_step_grid_target(self.handle, actions.data_ptr(), *self._step_out(), self._stream()),
                   "bbai_step_grid_target")
            return self._obs(rendered=True), self.reward, self.done, {}
        if self.view is not None and self.kernel_events is None:
            # ViewSizeWrapper's step: transition + the V x V view of every env as ONE call (include/bbai_view_size.h bbai_step_view)
            _check(self.lib, self.lib.bbai_step_view(self.handle, actions.data_ptr(), *self._step_out(), self.view_size, self.view.data_ptr(),
                                                     self._stream()), "bbai_step_view")
            return self._obs(rendered=True), self.reward, self.done, {}
        if self.pixel and not self.full_obs and self.tile_size == 8 and self.kernel_events is None and hasattr(self.lib, "bbai_step_render"):
            # the wrapped env's step: transition + render as ONE call (include/bbai.h bbai_step_render)
            _check(self.lib, self.lib.bbai_step_render(self.handle, actions.data_ptr(), *self._step_out(), self.pixels.data_ptr(), self._stream()),
                   "bbai_step_render")
            return self._obs(rendered=True), self.reward, self.done, {}
        _check(self.lib, self.lib.bbai_step(self.handle, actions.data_ptr(), *self._step_out(), self._stream()), "bbai_step")
        self._ev_end("step", ev)
        return self._obs(), self.reward, self.done, {}

    def step(self, actions, validate=None, ids=None):
        """env.step(actions[i]) for every env.  `ids` (an int sequence, an ndarray or an int64 device tensor of length k): step ONLY the listed
        envs -- `actions` has length k, env ids[j] takes actions[j] and every other env HOLDS (include/bbai.h BBAI_ACTION_HOLD): its state,
        step count and level stream stay, its observation rows are written again unchanged and its reward / done entries keep the values
        of its last step.  A 64-env block without a listed env costs one 64-byte load, so a sparse step costs little more than its launch.
        An id outside [0, num_envs) is skipped (pad with -1); a host list that names an env twice is a ValueError (in a device list it is
        undefined which action wins); a device list causes no host synchronisation.  Without `ids`, a full vector may carry HOLD bytes
        itself once set_option("step_hold", 1) is on.  Unknown actions: see validate_actions -- 8 is known exactly where it means hold."""
        if ids is None:
            actions = self._step_actions(actions, validate, self.num_envs, None)
            self._hold["actions"] = actions
            return self._step_native(actions)
        torch = self.torch
        self._no_env_twice("step", ids, padding=True)
        k, _, ids_t = self._ids(ids)
        actions = self._step_actions(actions, validate, k, True)
        n = self.num_envs
        buf = getattr(self, "_hold_actions", None)
        if buf is None:                 # uint8[N] full of HOLD between the calls, one spare entry behind it for the ids that name no env
            buf = self._hold_actions = torch.full((n + 1,), self.HOLD, dtype=torch.uint8, device=self.device)
        at = torch.where((ids_t < 0) | (ids_t >= n), n, ids_t)
        buf.index_copy_(0, at, actions)
        self._hold["actions"] = (buf, at, actions)
        before = self.get_option("step_hold")
        if before != 1:
            self.set_option("step_hold", 1)         # (a host value, read when the call below is enqueued: no synchronisation)
        try:
            return self._step_native(buf[:n])
        finally:
            if before != 1:
                self.set_option("step_hold", before)
            buf.index_fill_(0, at, self.HOLD)       # (behind the step on the same stream)

    def lookahead(self, ids, scratch):
        """Expand the states of the k listed envs with all seven actions, moving no other env and without a host trip: `scratch` = 7 k distinct
        envs of this batch, none of them listed, that the caller sets aside (their states are overwritten; ids in [0, num_envs)).  Scratch env
        7 j + a gets the state of env ids[j] (save_state / load_state) and takes action a in a step that every other env holds.  Returns the
        children's outputs, child (j, a) = env ids[j] after action a: {"image": the observation image (encoded, pixels or full, as step()
        returns it) [k, 7, ...], "direction", "reward", "reward64", "done": [k, 7]}.  The roots themselves do not move; a child whose
        episode ended shows the scratch env's own next level (auto_reset) and the terminal step's reward and done."""
        torch = self.torch
        self._no_env_twice("lookahead", scratch)
        if not isinstance(ids, torch.Tensor) and not isinstance(scratch, torch.Tensor):
            if set(np.asarray(ids, dtype=np.int64).reshape(-1).tolist()) & set(np.asarray(scratch, dtype=np.int64).reshape(-1).tolist()):
                raise ValueError("lookahead: a scratch env is one of the listed envs")
        k, _, ids_t = self._ids(ids)
        ks, _, scratch_t = self._ids(scratch)
        if ids_t is None or scratch_t is None or ks != 7 * k:
            raise ValueError("lookahead: %d scratch envs for %d listed envs (7 each)" % (ks, k))
        snap = self.save_state(ids_t)
        rows = torch.arange(k, dtype=torch.int64, device=self.device).repeat_interleave(7)
        self.load_state(snap, scratch_t, rows)
        acts = torch.arange(7, dtype=torch.uint8, device=self.device).repeat(k)
        obs = self.step(acts, validate=False, ids=scratch_t)[0]
        img = obs["image"].index_select(0, scratch_t)
        out = {"image": img.view((k, 7) + tuple(img.shape[1:]))}
        for name in ("direction", "reward", "reward64", "done"):
            out[name] = getattr(self, name).index_select(0, scratch_t).view(k, 7)
        return out

    def rollout(self, actions, tap=None, obs_row0=0, row0=0, step_tap=False):
        """An open-loop rollout (include/bbai.h bbai_rollout): `actions` uint8[T, N] on the device; T steps (+ the pixel render
        in pixel mode) are enqueued by ONE call, exactly what T calls of step() enqueue.  `tap`: a log dict as bench.py builds
        it -- device tensors "image" [rows, P, 7, 7, 3], "direction" [rows, P], "reward64" [rows, P], "done" [rows, P],
        optionally "pixels" [rows, PP, 56, 56, 3], and "ids" int64[P]: step t logs the listed envs' outputs into obs row
        obs_row0 + t / result row row0 + t.  Afterwards image / direction / reward / done (/ pixels) hold the last step's
        outputs; returns the observation dict of that step.  step_tap=True: the log's rows are written by the stepping lanes for the envs
        listed with set_step_tap() (log row k = listed env k; no "ids" needed, no pixel rows) -- with encoded observations one k_step launch then
        takes every step the look-ahead window has left (include/bbai.h bbai_rollout).  Under set_option("step_hold", 1) a HOLD byte holds
        its env for that tick, as in step()."""
        torch = self.torch
        if actions.dtype != torch.uint8 or actions.device != self.device or not actions.is_contiguous() or actions.dim() != 2 \
                or actions.shape[1] != self.num_envs:
            raise ValueError("actions: contiguous uint8[T, %d] on %s" % (self.num_envs, self.device))
        T = int(actions.shape[0])
        big = self.pixel and not self.full_obs and self.tile_size != 8        # tile sizes 16 / 32: encoded steps, the last frame drawn once
        if big and tap is not None and tap.get("pixels") is not None:
            raise ValueError("no pixel tap rows at tile size %d (only at 8)" % self.tile_size)
        log = None
        if tap is not None:
            P_ = int(tap["done"].shape[1])
            pix = tap.get("pixels")
            for k in ("image", "direction", "reward64", "done"):
                if not tap[k].is_contiguous():
                    raise ValueError("tap log tensors must be contiguous")
            if step_tap:
                pix = None
            log = TapLog(P_, int(pix.shape[1]) if pix is not None else 0, None if step_tap else tap["ids"].data_ptr(), tap["image"].data_ptr(), tap["direction"].data_ptr(),
                         tap["reward64"].data_ptr(), tap["done"].data_ptr(), pix.data_ptr() if pix is not None else None, int(obs_row0), int(row0))
            if tap["image"].shape[0] < obs_row0 + T or tap["done"].shape[0] < row0 + T:
                raise ValueError("tap log has too few rows for %d steps" % T)
        self._hold["actions"] = actions
        _check(self.lib, self.lib.bbai_rollout(self.handle, T, actions.data_ptr(), *self._step_out(),
                                                self.pixels.data_ptr() if self.pixels is not None and not big else None, ctypes.byref(log) if log is not None else None,
                                                self._stream()), "bbai_rollout")
        if big:
            self._render_batch_into(self.image, self.tile_size, self.pixels)
        if self.full_obs:
            self.observe_full()          # the last step's full observation (the tap log keeps its 7x7 rows)
        if self.view is not None:
            self.observe_view()          # the last step's view (the tap log keeps its 7x7 rows)
        return self._obs_dict(self.full if self.full_obs else self.view if self.view is not None else self.pixels if self.pixel else self.image)

    # ---- state access -------------------------------------------------------------------
    def programs(self, first=0, count=None):
        if not self.handle:
            raise EngineError("engine is closed (mission strings are fetched lazily: read them before close())")
        count = self.num_envs - first if count is None else count
        out = np.zeros((count, PROG_BYTES), dtype=np.uint8)
        _check(self.lib, self.lib.bbai_get_programs(self.handle, first, count, out.ctypes.data), "bbai_get_programs")
        return out

    def missions(self):
        return list(Missions(self))

    def export_state(self, first=0, count=None):
        count = self.num_envs - first if count is None else count
        rec = np.zeros((count, self.cfg.rec_bytes), dtype=np.uint8)
        hot = np.zeros((count, 16), dtype=np.uint8)
        stale = np.zeros((count,), dtype=np.uint64)
        _check(self.lib, self.lib.bbai_export_state(self.handle, first, count, rec.ctypes.data, hot.ctypes.data,
                                                     stale.ctypes.data), "bbai_export_state")
        return rec, hot, stale

    def grid_encoding(self, first=0, count=None):
        """uint8[count, W, H, 3]: the full-grid `env.grid.encode()` (type, colour, state per cell, indexed [x, y]) and
        the agent poses int[count, 3] = (x, y, dir) -- the `unwrapped.grid` / `agent_pos` view that the reference's own
        level test compares between same-seed envs (babyai/levels/levelgen.py:531-537)."""
        rec, hot, _ = self.export_state(first, count)
        c = self.cfg
        e = rec[:, :c.ES * c.EH].reshape(-1, c.EH, c.ES)[:, 5:5 + c.H, 5:5 + c.W].transpose(0, 2, 1)
        return np.stack([e & 7, (e >> 3) & 7, e >> 6], axis=-1).astype(np.uint8), hot[:, :3].astype(np.int64)

    def import_state(self, rec, hot, stale, first=0):
        """export_state()'s arrays into envs first .. first + len(rec) - 1 (include/bbai.h bbai_import_state; synchronous).  As after
        load_state the imported envs' next bot_actions() starts a fresh Bot and their `instr` rows hold the imported missions; unlike it, no
        observation is written: image / direction / pixels are stale until the next step."""
        rec = np.ascontiguousarray(rec, dtype=np.uint8)
        hot = np.ascontiguousarray(hot, dtype=np.uint8)
        stale = np.ascontiguousarray(stale, dtype=np.uint64)
        count = rec.shape[0]
        assert rec.shape == (count, self.cfg.rec_bytes) and hot.shape == (count, 16) and stale.shape == (count,)
        _check(self.lib, self.lib.bbai_import_state(self.handle, first, count, rec.ctypes.data, hot.ctypes.data,
                                                     stale.ctypes.data), "bbai_import_state")

    # ---- device snapshots (include/bbai.h bbai_save_state / bbai_load_state) -----------------------------------------
    def save_state(self, ids=None):
        """The live state of envs `ids` (None = every env; else an int sequence or an int64 device tensor, any order) as an EnvSnapshot on
        this batch's device: one launch on the current stream, no host trip.  Row k = env ids[k]; an id outside [0, num_envs) leaves its
        row zeroed."""
        torch = self.torch
        k, ids_ptr, self._hold["save_state"] = self._ids(ids)
        with torch.cuda.device(self.dev_index):
            u8 = dict(dtype=torch.uint8, device=self.device)
            snap = EnvSnapshot(torch.zeros((k, self.cfg.rec_bytes), **u8), torch.zeros((k, 16), **u8),
                               torch.zeros((k,), dtype=torch.int64, device=self.device), torch.zeros((k,), **u8),
                               self.env_id, self.cfg.rec_bytes, self.done_actions)
        _check(self.lib, self.lib.bbai_save_state(self.handle, ids_ptr, k, snap.rec.data_ptr(), snap.hot.data_ptr(), snap.stale.data_ptr(),
                                                   snap.lsm.data_ptr(), self._stream()), "bbai_save_state")
        return snap

    def _load_args(self, snap, ids, rows):
        """load_state's checks, before any device work: ValueError for a snapshot of another level, record size or done-action mode, for
        host-side `ids` with duplicates and for lists of different lengths."""
        if not isinstance(snap, EnvSnapshot):
            raise TypeError("load_state takes an EnvSnapshot")
        if snap.env_id != level_name(self.env_id):
            raise ValueError("snapshot of level %s loaded into a batch of %s" % (snap.env_id, level_name(self.env_id)))
        if snap.rec_bytes != self.cfg.rec_bytes:
            raise ValueError("snapshot with %d-byte records, this batch has %d" % (snap.rec_bytes, self.cfg.rec_bytes))
        if snap.done_actions != self.done_actions:
            raise ValueError("snapshot taken with done_actions=%s, this batch runs with done_actions=%s" % (snap.done_actions, self.done_actions))
        self._no_env_twice("load_state", ids)
        k = self.num_envs if ids is None else int(len(ids))
        kr = len(snap) if rows is None else int(len(rows))
        if rows is None and ids is None and kr < k:
            raise ValueError("load_state without ids and rows needs a snapshot of all %d envs, got %d rows" % (k, kr))
        if (rows is not None or ids is not None) and kr != k:
            raise ValueError("load_state: %d envs listed for %d rows" % (k, kr))

    def load_state(self, snap, ids=None, rows=None):
        """Put envs `ids` (None = every env) into the states of snapshot rows `rows` (None = row k into ids[k]; else an int sequence or an
        int64 device tensor, repeats allowed: one row may go into many envs) and return the observation dict as reset() does, the listed
        envs' rows holding gen_obs() of their loaded states.  One launch on the current stream (+ the batch's render in pixel /
        full_obs mode); no other env changes, and a loaded env goes on with its own next level when the loaded episode ends.  A snapshot
        on another device is copied over first.  ValueError: see _load_args; the same env twice in a DEVICE id list is undefined as to
        which row it gets."""
        torch = self.torch
        self._load_args(snap, ids, rows)
        if snap.device != self.device:
            snap = snap.to(self.device)
        tensors = tuple(t.contiguous() for t in (snap.rec, snap.hot, snap.stale, snap.lsm))
        if tensors[0].dtype != torch.uint8 or tensors[1].dtype != torch.uint8 or tensors[2].dtype != torch.int64 or tensors[3].dtype != torch.uint8:
            raise ValueError("snapshot tensors: uint8 rec / hot / lsm, int64 stale")
        k, ids_ptr, ids_t = self._ids(ids)
        _, rows_ptr, rows_t = self._ids(rows)
        self._hold["load_state"] = (tensors, ids_t, rows_t)
        _check(self.lib, self.lib.bbai_load_state(self.handle, ids_ptr, rows_ptr, k, len(snap), tensors[0].data_ptr(), tensors[1].data_ptr(),
                                                   tensors[2].data_ptr(), tensors[3].data_ptr(), self.image.data_ptr(),
                                                   self.direction.data_ptr(), self._stream()), "bbai_load_state")
        return self._obs()

    # ---- per-episode seeds (include/bbai.h bbai_reseed) ---------------------------------------------------------------
    def _reseed_args(self, ids, seeds):
        """reseed's checks and conversions, before the id list goes to the device: (k, seeds tensor int64[k] on the device).  ValueError for
        host-side `ids` that list an env twice, for lists of different lengths and for seeds outside uint64 ("negative")."""
        torch = self.torch
        self._no_env_twice("reseed", ids, padding=True)
        k = self.num_envs if ids is None else int(len(ids))
        if isinstance(seeds, torch.Tensor):
            if seeds.dim() != 1 or seeds.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)) or seeds.device != self.device:
                raise ValueError("seeds: int64 / uint64 [k] on %s" % (self.device,))
            seeds_t = seeds.contiguous().view(torch.int64)          # (the same bits; the device does not check their sign)
        else:
            host = seeds_u64(seeds, "reseed")
            seeds_t = torch.as_tensor(host.view(np.int64), device=self.device) if len(host) else torch.zeros((0,), dtype=torch.int64, device=self.device)
        if int(seeds_t.shape[0]) != k:
            raise ValueError("reseed: %d envs listed for %d seeds" % (k, int(seeds_t.shape[0])))
        return k, seeds_t

    def reseed(self, ids, seeds, levels=None):
        """`env[ids[k]].seed(seeds[k]); env[ids[k]].reset()` for the listed envs of a live batch (ids None = every env; an int sequence,
        an ndarray or an int64 device tensor; seeds: ints, a uint64 ndarray or an int64 / uint64 device tensor), on the current stream
        without a host synchronisation: each listed env's level stream restarts from its seed, the env starts level 0 of it -- a frozen
        env (auto_reset=False) is live again -- and every other env goes on as if nothing had happened.  Returns the observation dict as
        reset() does, the listed rows holding the new episodes' first observations.  An id outside [0, num_envs) is skipped (pad with
        -1); ValueError: see _reseed_args; the same env twice in a DEVICE id list is undefined as to which seed it gets.
        `levels`: how many levels of its new stream a listed env will play (include/bbai.h bbai_reseed, option "reseed_levels"): only those
        are generated, and the env PARKS -- frozen, done = 1, its other outputs unspecified -- when the last of them ends, until it is
        reseeded again.  None: the handle's option as it stands (0 unless set: the whole look-ahead ring, the env never parks); an int: that
        depth for this call, the option's previous value put back behind it; 0 or anything beyond the ring's depth is the whole ring.
        ValueError for a negative or non-integer value."""
        levels = reseed_levels_arg(levels, "reseed")
        k, seeds_t = self._reseed_args(ids, seeds)
        if k == 0:
            return self._obs()
        _, ids_ptr, ids_t = self._ids(ids)
        self._hold["reseed"] = (ids_t, seeds_t)
        before = None if levels is None else self.get_option("reseed_levels")
        if before is not None and before != levels:
            self.set_option("reseed_levels", levels)
        try:
            _check(self.lib, self.lib.bbai_reseed(self.handle, ids_ptr, seeds_t.data_ptr(), k, self.image.data_ptr(), self.direction.data_ptr(),
                                                   self._stream()), "bbai_reseed")
        finally:
            if before is not None and before != levels:
                self.set_option("reseed_levels", before)
        return self._obs()

    def save_checkpoint(self):
        """The whole batch as one host blob (np.uint8): live state, RNG streams, look-ahead ring, window bookkeeping,
        counters, the expert's plans -- everything `load_checkpoint` needs to continue bit-identically."""
        nbytes = int(self.lib.bbai_checkpoint_bytes(self.handle))
        blob = np.empty(nbytes, dtype=np.uint8)
        _check(self.lib, self.lib.bbai_checkpoint_save(self.handle, blob.ctypes.data, nbytes), "bbai_checkpoint_save")
        return blob

    def load_checkpoint(self, blob):
        """Continue a saved run in this handle (same level, batch size and look-ahead depth).  The current observation
        is not part of the blob: callers that need it keep `image` / `direction` next to it (or step once)."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        _check(self.lib, self.lib.bbai_checkpoint_load(self.handle, blob.ctypes.data, blob.size), "bbai_checkpoint_load")
        if self.instr is not None:        # refill the caller-owned token rows from the loaded programs
            _check(self.lib, self.lib.bbai_set_token_buffer(self.handle, self.instr.data_ptr()), "bbai_set_token_buffer")

    def enable_instr_tokens(self):
        """Keep `self.instr` (uint8[N, 72] on the device) filled with the mission token ids of the current
        episodes -- the tensor fast path that replaces per-step regex tokenisation (format.py:59-75)."""
        if self.instr is None:
            with self.torch.cuda.device(self.dev_index):
                self.instr = self.torch.zeros((self.num_envs, TOK_MAX), dtype=self.torch.uint8, device=self.device)
            _check(self.lib, self.lib.bbai_set_token_buffer(self.handle, self.instr.data_ptr()), "bbai_set_token_buffer")
        return self.instr

    BOT_GAVE_UP = 255
    RESET_ENV = 7          # step() "action": abandon the episode of that env (include/bbai.h BBAI_ACTION_RESET_ENV)
    HOLD = 8               # step() "action" under set_option("step_hold", 1) / step(ids=...): this env sits the step out (BBAI_ACTION_HOLD)

    def bot_actions(self, prev_actions=None, out=None):
        """One decision of the reference's expert (babyai/bot.py Bot.replan) for every env, on the device:
        uint8[N] suggested actions, BOT_GAVE_UP (255) where the reference bot would have raised.  `prev_actions` = the
        actions the envs were really stepped with since the last call (advising mode), None = the suggestions."""
        torch = self.torch
        self._expert_sees_7x7("bot_actions")
        if out is None:
            if self._bot_out is None:
                self._bot_out = torch.zeros((self.num_envs,), dtype=torch.uint8, device=self.device)
            out = self._bot_out
        prev_ptr = None
        if prev_actions is not None:
            if not isinstance(prev_actions, torch.Tensor):
                prev_actions = torch.as_tensor(np.asarray(prev_actions), device=self.device)
            prev_actions = prev_actions.to(device=self.device, dtype=torch.uint8).contiguous()
            if prev_actions.numel() != self.num_envs:
                raise ValueError("need %d previous actions" % self.num_envs)
            self._hold["bot_act"] = prev_actions
            prev_ptr = prev_actions.data_ptr()
        _check(self.lib, self.lib.bbai_bot_act(self.handle, prev_ptr, out.data_ptr(), self._stream()), "bbai_bot_act")
        return out

    def bot_rollout(self, steps, tokens=False, out=None):
        """`steps` expert decisions + auto-reset steps for every env with no host round trip in between (include/bbai.h
        bbai_bot_rollout: the inner loop of scripts/make_agent_demos.py:71-137).  Returns device tensors [steps, N, ...]:
        image / direction (and tokens, uint8[steps, N, 72] mission token ids, if asked) = what the expert decided on at
        each step, action = its decision (RESET_ENV where it gave up: gave_up = 1), reward, done = the step's results.
        Afterwards self.image / self.direction hold the current observation as after step().  `out`: a dict of such tensors (what an earlier
        call returned, or preallocated ones of the same shapes and types) to write into instead of fresh ones -- a history slot that is
        reused allocates nothing."""
        torch = self.torch
        T, n = int(steps), self.num_envs
        self._expert_sees_7x7("bot_rollout")
        if not self.auto_reset:
            raise EngineError("bot_rollout steps with ParallelEnv semantics: construct the env with auto_reset=True")
        shapes = {"image": (T, n, 7, 7, 3), "direction": (T, n), "action": (T, n), "reward": (T, n), "done": (T, n), "gave_up": (T, n)}
        if tokens:
            shapes["tokens"] = (T, n, TOK_MAX)
        if out is not None:
            for k, shape in shapes.items():
                t = out.get(k)
                if t is None or tuple(t.shape) != shape or t.dtype != (torch.float32 if k == "reward" else torch.uint8) or t.device != self.device \
                        or not t.is_contiguous():
                    raise ValueError("bot_rollout: out[%r] must be a contiguous %s%s on %s" % (k, "float32" if k == "reward" else "uint8", list(shape), self.device))
            if tokens:
                self.enable_instr_tokens()
        else:
            with torch.cuda.device(self.dev_index):
                out = {k: torch.empty(shape, dtype=torch.float32 if k == "reward" else torch.uint8, device=self.device) for k, shape in shapes.items()}
                if tokens:
                    self.enable_instr_tokens()
        tok_ptr = out["tokens"].data_ptr() if tokens else None
        _check(self.lib, self.lib.bbai_bot_rollout(self.handle, T, self.image.data_ptr(), self.direction.data_ptr(),
                                                    out["image"].data_ptr(), out["direction"].data_ptr(), tok_ptr,
                                                    out["action"].data_ptr(), out["reward"].data_ptr(), out["done"].data_ptr(),
                                                    out["gave_up"].data_ptr(), self._stream()), "bbai_bot_rollout")
        self._moved_on()
        return out

    def bot_stats(self):
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(self.lib, self.lib.bbai_bot_stats(self.handle, ctypes.byref(a), ctypes.byref(b)), "bbai_bot_stats")
        return {"gave_up": int(a.value), "capacity": int(b.value)}

    def tap(self, image_out, dir_out, reward64_out, done_out, pixels_out=None, ids=None):
        """Copy the current outputs of the first len(done_out) envs -- or of the envs `ids` (int64 device tensor, any order)
        -- into the given log rows, and the pixels of the first len(pixels_out) of them, with one launch on the current
        stream (bench.py's in-run parity tap)."""
        pp = 0 if pixels_out is None else int(pixels_out.shape[0])
        if self.torch.cuda.current_device() != self.dev_index:      # handle-free entry point: launches on the CURRENT device
            with self.torch.cuda.device(self.dev_index):
                return self.tap(image_out, dir_out, reward64_out, done_out, pixels_out, ids)
        count = int(done_out.shape[0])
        src = (self.image.data_ptr(), self.direction.data_ptr(), self.reward64.data_ptr(), self.done.data_ptr(),
               self.pixels.data_ptr() if pp else None)
        dst = (image_out.data_ptr(), dir_out.data_ptr(), reward64_out.data_ptr(), done_out.data_ptr(),
               pixels_out.data_ptr() if pp else None, self._stream())
        if ids is None:
            _check(self.lib, self.lib.bbai_tap(count, pp, *src, *dst), "bbai_tap")
        else:
            if ids.dtype != self.torch.int64 or ids.device != self.device or ids.numel() != count or not ids.is_contiguous():
                raise ValueError("ids: contiguous int64[%d] on %s" % (count, self.device))
            _check(self.lib, self.lib.bbai_tap_ids(count, pp, ids.data_ptr(), *src, *dst), "bbai_tap_ids")

    def set_step_tap(self, ids):
        """The envs step_tapped() logs (include/bbai.h bbai_step_tap_set): any order, no duplicates; log row k = env ids[k].  None / empty clears."""
        ids = np.ascontiguousarray(np.asarray([] if ids is None else ids, dtype=np.int64))
        _check(self.lib, self.lib.bbai_step_tap_set(self.handle, ids.ctypes.data if len(ids) else None, len(ids)), "bbai_step_tap_set")
        self._step_tap = len(ids)

    def step_tapped(self, actions, image_out, dir_out, reward64_out, done_out):
        """step(actions) + the listed envs' outputs of this step into the given log rows (uint8[count, 7, 7, 3], uint8[count], float64[count],
        uint8[count] on the device) -- written by the stepping lanes themselves, no launch behind the step (include/bbai.h bbai_step_tapped).
        `actions`: uint8[num_envs] on the device."""
        if actions.dtype != self.torch.uint8 or actions.device != self.device or not actions.is_contiguous() or actions.numel() != self.num_envs:
            raise ValueError("actions: contiguous uint8[%d] on %s" % (self.num_envs, self.device))
        if int(done_out.shape[0]) != self._step_tap:
            raise ValueError("log rows for %d envs, set_step_tap() listed %d" % (int(done_out.shape[0]), self._step_tap))
        self._hold["actions"] = actions
        _check(self.lib, self.lib.bbai_step_tapped(self.handle, actions.data_ptr(), *self._step_out(), image_out.data_ptr(), dir_out.data_ptr(),
                                                    reward64_out.data_ptr(), done_out.data_ptr(), self._stream()), "bbai_step_tapped")
        self._moved_on()
        return self.reward, self.done

    def set_call_events(self, enable=True):
        """Record the handle's completion event at the end of every call, so that a caller may destroy a stream it used
        for this env and come back on another one (include/bbai.h bbai_set_call_events; off by default: ~3 us per call)."""
        _check(self.lib, self.lib.bbai_set_call_events(self.handle, 1 if enable else 0), "bbai_set_call_events")

    def set_option(self, name, value):
        """A performance knob of the live handle by name (include/bbai.h bbai_set_option: launch shapes, render input,
        priorities -- never semantics, but for "done_action_enum", "reseed_levels" (see reseed()) and "step_hold" (see step())).  What measurements alternate inside
        one process (tools/ab.py)."""
        _check(self.lib, self.lib.bbai_set_option(self.handle, name.encode(), int(value)), "bbai_set_option(%s)" % name)
    
    def get_option(self, name):
        """A knob of the live handle (the names of set_option), or "lookahead_period" (the refill period chosen at create)."""
        v = ctypes.c_int64(0)
        _check(self.lib, self.lib.bbai_get_option(self.handle, name.encode(), ctypes.byref(v)), "bbai_get_option(%s)" % name)
        return int(v.value)

    def _has_option(self, name):
        """Does the loaded library know option `name` (an older experiment build, BBAI_ENGINE_LIB, may not)."""
        v = ctypes.c_int64(0)
        return self.lib.bbai_get_option(self.handle, name.encode(), ctypes.byref(v)) == 0

    def profile(self, enable=True):
        """Bracket every k_step / k_consume / k_render launch with HIP events on its launch stream (bench.py)."""
        _check(self.lib, self.lib.bbai_profile(self.handle, 1 if enable else 0), "bbai_profile")

    def profile_resume(self):
        """Bracket launches again, adding to the totals kept since profile(True)."""
        _check(self.lib, self.lib.bbai_profile(self.handle, 2), "bbai_profile")

    def profile_pause(self):
        """Stop bracketing launches; the totals stay readable."""
        _check(self.lib, self.lib.bbai_profile(self.handle, 0), "bbai_profile")

    def profile_read(self):
        """{kernel: (average ms per launch, launches)} since profile(True)."""
        ms = (ctypes.c_double * 3)()
        cnt = (ctypes.c_int64 * 3)()
        _check(self.lib, self.lib.bbai_profile_read(self.handle, ms, cnt), "bbai_profile_read")
        return {k: (ms[i] / cnt[i] if cnt[i] else None, int(cnt[i])) for i, k in enumerate(("k_step", "k_consume", "k_render"))}

    def reset_count(self):
        v = ctypes.c_uint64(0)
        _check(self.lib, self.lib.bbai_reset_count(self.handle, ctypes.byref(v)), "bbai_reset_count")
        return int(v.value)

    def generator_failures(self):
        v = ctypes.c_uint64(0)
        _check(self.lib, self.lib.bbai_generator_failures(self.handle, ctypes.byref(v)), "bbai_generator_failures")
        return int(v.value)

    def max_steps(self):
        """Per-env max_steps of the current episodes (levelgen.py:42-45)."""
        _, hot, _ = self.export_state()
        return hot[:, 6].astype(np.int32) | (hot[:, 7].astype(np.int32) << 8)

    def gate_timeouts(self):
        """Window gates that gave up waiting for a look-ahead refill (bbai_ring.hpp k_gate): must be 0 -- anything else means a
        refill was lost and the batch's results are void.  Synchronises."""
        return self.get_option("gate_timeouts")

    def gate_fault(self):
        """The sticky flag a timed-out window gate leaves in pinned host memory (no synchronisation).  Once it is set, step() / reset() /
        rollout() raise EngineError at the next call (the C entry points return BBAI_ERR_STATE) -- the error surfaces where it happens, not
        at close()."""
        return bool(self.get_option("gate_fault"))

    def close(self):
        """Destroy the handle.  A gate time-out is reported by the stepping calls themselves (gate_fault); close() only warns about one that
        no later call had the chance to report -- it never raises over an exception that is already in flight."""
        if getattr(self, "handle", None) is not None and self.handle:
            fault = False
            try:
                fault = self.gate_fault()
            except Exception:
                pass
            self.lib.bbai_destroy(self.handle)
            self.handle = ctypes.c_void_p()
            if fault and sys.exc_info()[0] is None:
                raise EngineError("a window gate of this batch timed out waiting for a look-ahead refill: the results since are void")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
