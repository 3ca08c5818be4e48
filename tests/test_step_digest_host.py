"""Stepping and the verifier against digests RECORDED FROM THE REFERENCE at scale (tests/golden/refpin/step_digest/, tools/gen_golden_refpin.py
step): every registered kind, 256 streams seeded 53000 + i, 128 steps in one room and 320 in several, with auto-reset, under the reference's
own expert with 8 % random actions -- so that episodes end in success -- and a digest per stream and 16-step block over every observation,
direction, float64 reward and done (refpin_util.step_block_digests).  The recorded actions are replayed on

  - the engine's host build in k_step's order of operations (bbai_step.hpp step_env_prefetch through HostBatch): the whole fixture;
  - the same headers in the reference's order of operations (hs_step64), on the eight kinds of test_gpu_step_every_level.SUBSET;
  - the oracle (oracle/levels.py) through the protocol function the recorder ran: streams 0 .. 31, all 256 with BBAI_STEP_DIGEST_FULL=1;
  - the host build's expert (bbai_bot.hpp): the recorded action wherever it was the reference expert's own suggestion, "gave up" where the
    reference's expert raised -- 256 streams per kind where tests/golden/bot/ holds 6 to 8.

No build of this project stands between the fixture and what is tested; tests/test_gpu_step_digest.py does the same on the device and
tests/test_step_digest_sanitized.py in a sanitized stand-alone program."""
import ctypes
import os

import numpy as np
import pytest

import refpin_util as rp
from babyai_amd.levels import LEVELS, make_cfg
from hostsim_util import HostBatch, HostEnv, lib
from test_gpu_step_every_level import SUBSET

S, SEED0, B = rp.STEP_DIGEST_STREAMS, rp.STEP_DIGEST_SEED0, rp.STEP_DIGEST_BLOCK
ORACLE_STREAMS = S if os.environ.get("BBAI_STEP_DIGEST_FULL") == "1" else 32
# The reference's subgoal list is unbounded, and an expert in an unproductive loop grows it by about four entries every five steps until the
# time limit (tests/test_hostsim_bot.py test_stack_capacity_is_the_one_documented_divergence: the default 48 entries give up there).  With room
# for any stack that T steps can build, the host expert has to follow the reference's all the way.
STACK_CAP = 1024


def _host_replay(name, fx, expert=False):
    """The recorded actions on HostBatch -> (first digests, block digests, done [T, S], the expert's suggestions uint8[T, S] or None)."""
    cfg, acts = make_cfg(name), fx["actions"]
    steps = acts.shape[0]
    hb = HostBatch(cfg, SEED0 + np.arange(S))
    hb.reset()
    first = rp.step_first_digests(hb.image, hb.direction)
    image, direction = np.zeros((steps, S, 7, 7, 3), np.uint8), np.zeros((steps, S), np.uint8)
    reward, done = np.zeros((steps, S), np.float64), np.zeros((steps, S), np.uint8)
    sug = None
    if expert:
        L = lib()
        L.hs_bot_set_eager(1)
        sug = np.full((steps, S), 255, np.uint8)
        state = np.zeros((S, L.hs_bot_state_bytes(STACK_CAP)), np.uint8)
        args = [(ctypes.byref(cfg), hb.rec[i].ctypes.data, hb.hot[i].ctypes.data, hb.stale[i:].ctypes.data, state[i].ctypes.data, STACK_CAP) for i in range(S)]
        fresh, alive, last = [1] * S, [True] * S, [-1] * S
    try:
        for t in range(steps):
            if expert:
                row = acts[t].tolist()
                for i in range(S):
                    if alive[i]:
                        a = L.hs_bot_decide(*args[i], fresh[i], last[i])
                        sug[t, i], alive[i], fresh[i] = a, a != 255, 0
                    last[i] = row[i]
            hb.step(acts[t])
            image[t], direction[t], reward[t], done[t] = hb.image, hb.direction, hb.reward64, hb.done
            if expert:
                for i in np.nonzero(hb.done)[0]:
                    state[i] = 0
                    fresh[i], alive[i], last[i] = 1, True, -1
    finally:
        if expert:
            L.hs_bot_set_eager(0)
    return first, rp.step_block_digests(image, direction, reward, done), done, sug


@pytest.mark.parametrize("name", sorted(LEVELS))
def test_host_build_reproduces_the_reference_digests(name):
    fx = rp.step_digest_fixture(name)
    first, got, _, _ = _host_replay(name, fx)
    rp.step_digest_mismatch(name, first, got, fx, "host build, k_step's order")


@pytest.mark.parametrize("name", SUBSET)
def test_reference_order_reproduces_the_reference_digests(name):
    fx = rp.step_digest_fixture(name)
    cfg, acts = make_cfg(name), fx["actions"]
    steps = acts.shape[0]
    image, direction = np.zeros((steps, S, 7, 7, 3), np.uint8), np.zeros((steps, S), np.uint8)
    reward, done = np.zeros((steps, S), np.float64), np.zeros((steps, S), np.uint8)
    first_image, first_direction = np.zeros((S, 7, 7, 3), np.uint8), np.zeros(S, np.uint8)
    for i in range(S):
        env = HostEnv(cfg, SEED0 + i)
        assert not env.prefetch_order
        first_image[i], first_direction[i] = env.reset(), env.hot[2]
        for t, a in enumerate(acts[:, i].tolist()):
            img, _, d = env.step(a)
            if d:
                img = env.reset()
            image[t, i], direction[t, i], reward[t, i], done[t, i] = img, env.hot[2], env.last_reward64, d
    rp.step_digest_mismatch(name, rp.step_first_digests(first_image, first_direction), rp.step_block_digests(image, direction, reward, done), fx,
                            "host build, the reference's order (hs_step64)")


@pytest.mark.parametrize("name", sorted(LEVELS))
def test_oracle_reproduces_the_reference_digests(name):
    from oracle import levels as olevels
    fx = rp.step_digest_fixture(name)

    def env_for_seed(seed):
        e = olevels.make_env(name)
        e.seed(seed)
        return e
    o = rp.step_digest_run(env_for_seed, range(ORACLE_STREAMS), fx["actions"].shape[0], lambda i: rp.RecordedActions(fx["actions"][:, i]))
    rp.step_digest_mismatch(name, rp.step_first_digests(o["first_image"], o["first_direction"]),
                            rp.step_block_digests(o["image"], o["direction"], o["reward"], o["done"]), fx, "oracle", streams=np.arange(ORACLE_STREAMS))
    assert np.array_equal(o["ends"], fx["ends"][:ORACLE_STREAMS]), name       # (how the episodes ended: success, failure, time limit)


@pytest.mark.parametrize("name", sorted(LEVELS))
def test_host_expert_reproduces_the_reference_expert(name):
    fx = rp.step_digest_fixture(name)
    first, got, done, sug = _host_replay(name, fx, expert=True)
    rp.step_digest_mismatch(name, first, got, fx, "host build under the expert's reads")
    own, raised = rp.step_digest_expert(name, "host expert", sug, done, fx)
    assert own == int((fx["suggested"] & ~fx["bot_dead"]).sum()) and own > 0, (name, own)


def test_fixture_is_complete():
    d = rp.golden_path("step_digest")
    assert sorted(f[:-4] for f in os.listdir(d) if f.endswith(".npz")) == sorted(LEVELS)
    assert len(LEVELS) == 105
    for name in sorted(LEVELS):
        fx = rp.step_digest_fixture(name)
        steps = rp.step_digest_steps(name)
        assert steps % B == 0
        assert fx["actions"].shape == (steps, S) and fx["actions"].dtype == np.uint8 and fx["actions"].max() <= 6, name
        assert fx["digest"].shape == (S, steps // B) and fx["digest"].dtype == np.uint32, name
        assert fx["first"].shape == (S,) and fx["first"].dtype == np.uint32, name
        assert fx["suggested"].shape == fx["bot_dead"].shape == (steps, S), name
        assert not (fx["suggested"] & fx["bot_dead"]).any(), name
        assert fx["ends"].shape == (S, 3) and fx["budget"].ndim == 2 and fx["budget"].shape[1] == 2, name
        assert all(fx["bot_dead"][t, i] for t, i in fx["budget"]), name
        with np.load(rp.golden_path(os.path.join("step_digest", name + ".npz"))) as z:
            assert z["actions"].shape == (steps, S // 2) and z["suggested"].shape == z["bot_dead"].shape == (steps, S // 8), name


def test_pack_and_unpack():
    rng = np.random.RandomState(3)
    a = rng.randint(0, 7, size=(9, 10)).astype(np.uint8)
    assert np.array_equal(rp.unpack_actions(rp.pack_actions(a)), a) and rp.pack_actions(a).shape == (9, 5)
    bits = rng.rand(9, 16) < 0.5
    assert np.array_equal(rp.unpack_bits(rp.pack_bits(bits), 16), bits) and rp.pack_bits(bits).shape == (9, 2)


def test_digest_sees_every_field():
    rng = np.random.RandomState(5)
    n, steps = 2, 2 * B
    base = dict(image=rng.randint(0, 256, size=(steps, n, 7, 7, 3)).astype(np.uint8), direction=rng.randint(0, 4, size=(steps, n)).astype(np.uint8),
                reward=rng.rand(steps, n), done=(rng.rand(steps, n) < 0.2).astype(np.uint8))
    d0 = rp.step_block_digests(**base)
    assert d0.shape == (n, 2) and d0.dtype == np.uint32 and np.array_equal(d0, rp.step_block_digests(**base))
    assert len(np.unique(d0)) == 4

    def only(stream, block, **kw):
        """The change moves the digest of that (stream, block) and no other."""
        d = rp.step_block_digests(**dict(base, **kw))
        want = np.zeros((n, 2), bool)
        want[stream, block] = True
        assert np.array_equal(d != d0, want), (kw.keys(), stream, block)

    for t, i, at in ((0, 0, (0, 0, 0)), (B - 1, 1, (6, 6, 2)), (B, 0, (3, 6, 1)), (steps - 1, 1, (0, 3, 2))):      # one observation byte
        im = base["image"].copy()
        im[(t, i) + at] ^= 1
        only(i, t // B, image=im)
    for t, i in ((0, 1), (B - 1, 0), (B, 1), (steps - 1, 0)):
        dr = base["direction"].copy()
        dr[t, i] ^= 1
        only(i, t // B, direction=dr)
        rw = base["reward"].copy()
        rw[t, i] = np.nextafter(rw[t, i], 2.0)                    # the last bit of the mantissa
        assert rw[t, i] != base["reward"][t, i] and np.float32(rw[t, i]) == np.float32(base["reward"][t, i])
        only(i, t // B, reward=rw)
        dn = base["done"].copy()
        dn[t, i] ^= 1
        only(i, t // B, done=dn)
    # the same bytes in another step order: two steps of a block swapped
    swap = {k: v.copy() for k, v in base.items()}
    for v, w in zip(swap.values(), base.values()):
        v[3, 0], v[7, 0] = w[7, 0], w[3, 0]
    d = rp.step_block_digests(**swap)
    assert d[0, 0] != d0[0, 0] and d[0, 1] == d0[0, 1] and np.array_equal(d[1], d0[1])
    # ... and two whole blocks with each other's bytes swap their digests
    swap = {k: np.concatenate([v[B:], v[:B]]) for k, v in base.items()}
    assert np.array_equal(rp.step_block_digests(**swap), d0[:, ::-1])
    # the first observation's digest
    f0 = rp.step_first_digests(base["image"][0], base["direction"][0])
    im = base["image"][0].copy()
    im[1, 6, 6, 2] ^= 1
    assert np.array_equal(rp.step_first_digests(im, base["direction"][0]) != f0, [False, True])
    assert np.array_equal(rp.step_first_digests(base["image"][0], base["direction"][0] ^ np.uint8(2)) != f0, [True, True])
