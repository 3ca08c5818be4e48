"""The stand-alone oracle against the REFERENCE ITSELF (babyai imported unmodified on the restated gym_minigrid shim), through
records of the reference taken by tools/gen_golden_refpin.py (tests/golden/refpin/): the oracle replays the same seeds and the
same actions and must produce the same missions, time limits, grids, observations, rewards and dones.  Only
test_c1_digest_from_the_reference_itself still imports the reference: it re-derives a committed constant, where the tree exists."""
import types

import numpy as np
import pytest

from oracle import refenv
from oracle import levels as olevels
import refpin_util as rp


@pytest.fixture(scope="module")
def levels_record():
    return rp.load_json("levels.json")


@pytest.fixture(scope="module")
def episodes_record():
    return rp.load_json("random_episodes.json")


@pytest.mark.parametrize("name", sorted(olevels.SPECS))
def test_oracle_vs_reference(episodes_record, name):
    def env_for_seed(seed):
        ora = olevels.make_env(name)
        ora.seed(seed)
        return ora

    got, want = rp.random_episodes(env_for_seed), episodes_record[name]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (name, w["seed"], w["ep"])


def test_reference_constructor_args_match_table(levels_record):
    """The level table restates the reference constructors: compare against the attributes of reference objects."""
    for name, (fam, kw) in olevels.SPECS.items():
        ref = types.SimpleNamespace(**levels_record["attrs"][name])
        if fam == "fixed":
            assert (ref.room_size, ref.num_rows, ref.num_cols) == (kw.get("room_size", 9), kw.get("num_rows", 1), kw.get("num_cols", 1))
            continue
        assert ref.room_size == kw.get("room_size", 8), name
        assert ref.num_rows == kw.get("num_rows", 1 if fam == "goto" else 3), name
        assert ref.num_cols == kw.get("num_cols", 1 if fam == "goto" else 3), name
        if fam == "bonus":
            if hasattr(ref, "objs_per_room"):
                assert ref.objs_per_room == kw["num_dists"], name
            if hasattr(ref, "num_doors"):
                assert ref.num_doors == kw["sp"][0], name
            if hasattr(ref, "debug"):
                assert bool(ref.debug) == bool(kw["sp"][-1]), name
            if hasattr(ref, "start_carrying"):
                assert bool(ref.start_carrying) == bool(kw["sp"][0]), name
            continue
        if fam == "levelgen":
            assert list(ref.action_kinds) == list(kw.get("action_kinds", ("goto", "pickup", "open", "putnext")))
            assert list(ref.instr_kinds) == list(kw.get("instr_kinds", ("action", "and", "seq")))
            assert ref.locked_room_prob == kw.get("locked_room_prob", 0.5)
            assert ref.num_dists == kw.get("num_dists", 18)
            for k, d in (("locations", True), ("unblocking", True), ("implicit_unlock", True)):
                assert bool(getattr(ref, k)) == bool(kw.get(k, d))
        elif hasattr(ref, "num_dists"):
            assert ref.num_dists == kw.get("num_dists", 8)
        elif hasattr(ref, "num_objs"):
            assert ref.num_objs == kw.get("num_dists", 8)


def test_reference_own_smoke_test_passes_on_shim(levels_record):
    """A trimmed run of the reference's only test of this path (babyai/levels/levelgen.py:496-541) -- surface/mission agreement
    and same-seed determinism for every registered level -- on the oracle, whose seed-0 levels and first missions must be the
    reference's."""
    for name, rec in levels_record["seed0"].items():
        m0, m1 = olevels.make_env(name, seed=0), olevels.make_env(name, seed=0)
        assert isinstance(m0.surface, str) and len(m0.surface) > 0
        assert m0.unwrapped.grid == m1.unwrapped.grid and m0.surface == m1.surface
        grid = rp.Digest()
        grid.add(m0.unwrapped.grid.encode(), np.uint8)
        assert (m0.surface, grid.hexdigest()) == (rec["surface"], rec["grid"]), name
        obs = m0.reset()
        assert obs["mission"] == m0.surface == rec["reset_mission"], name


def test_level_table_covers_every_registered_level(levels_record):
    """All 105 ids the reference registers (levelgen.py:467-493) are in the engine's and the oracle's tables."""
    from babyai_amd.levels import LEVELS
    assert len(levels_record["registered"]) == 105
    assert set(levels_record["registered"]) == set(LEVELS) == set(olevels.SPECS)


@pytest.mark.skipif(not refenv.have_reference(), reason="reference tree not present (tests/test_oracle_golden.py pins the oracle to the same digest)")
def test_c1_digest_from_the_reference_itself():
    from oracle import cpu_baseline
    from test_oracle_golden import C1_DIGEST
    assert cpu_baseline.c1(use_reference=True)["digest"] == C1_DIGEST
