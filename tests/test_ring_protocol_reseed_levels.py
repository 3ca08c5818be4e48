"""The look-ahead ring's window protocol with SHORT reseeds (bbai_reseed under option "reseed_levels" = k, babyai_amd/csrc/bbai_reseedk.hpp;
DESIGN.md section 5g), as a model: host logic, no GPU.  The model of tests/test_ring_protocol_reseed.py (its own copy here) with a depth per
reseed.  A reseed of env i at depth k (0 < k < fill; fill = D, or D - 1 in place)

  * waits for every refill launched so far, clears the env's byte in the current window's buffer and consumes slot 0, booked into the current
    window, exactly as a whole-ring reseed does;
  * puts levels 0 .. k - 1 of a NEW sequence into slots 0 .. k - 1 and the empty frozen state into every slot's hot entry: slot k is the PARKING
    slot, and the slots behind it keep whatever record they held (STALE: an older level; nothing is booked for them);
  * the env's ordinary move into slot k -- booked like any other -- PARKS it: it never moves again until a reseed.

Checked, under refills that land as late as the gate allows or at random moments: an env finds the levels of its current sequence in order and
then its parking slot; no slot is read while a refill for it is in flight; no refill lands on a slot that holds an unplayed level, the parking
slot of an env that has not reached it, or (in place) the live slot -- a parked env's included; a window's `pending` stays a byte (at most
B + 1); a parked env stays parked whatever the ticks say; the envs that are not reseeded go on as if nothing had happened."""
import numpy as np
import pytest

NWIN = 34            # bbai_kernels.hpp NWIN
PARK, STALE = ("park",), ("stale",)


class Env:
    """One env's ring under the engine's bookkeeping; a level is (sequence it belongs to, number in it)."""

    def __init__(self, B, depth, inplace, nwin):
        self.B, self.D, self.inplace = B, depth, inplace
        self.fill = depth - 1 if inplace else depth
        self.epoch = 0
        self.busy = [False] * depth
        self.pending = [0] * nwin
        self.first_slot = [0] * nwin
        self.early = 0
        self.total_played = 0
        self.parkings = 0
        self.level = [None] * depth
        self._new_ring(0)

    def _new_ring(self, k):
        gen = k if 0 < k < self.fill else self.fill          # k_reseed_seed: rs_pending
        old = self.level
        self.level = [(self.epoch, s) if s < gen else PARK if s == gen and gen < self.fill else STALE if s < self.fill else None for s in range(self.D)]
        if self.inplace and gen < self.fill and old[self.D - 1] is not None:
            self.level[self.D - 1] = STALE                  # (the in-place layout's slot D - 1 keeps its record too; the reseed's consume frees it)
        self.gen_seq = gen
        self.limit = gen if gen < self.fill else None       # levels the env may play before it parks
        self.next = 0
        self.played = 0
        self.parked = False

    def live(self):
        return (self.next - 1) % self.D

    def finish(self, wb):
        assert not self.parked, "a parked env moved"
        s = self.next
        assert not self.busy[s], "the env moved to a slot whose refill has not landed"
        if self.limit is not None and self.played == self.limit:
            assert self.level[s] == PARK, "the env did not find its parking slot behind its last level"
            self.parked = True
            self.parkings += 1
        else:
            assert self.level[s] == (self.epoch, self.played), "the env did not get the next level of its current sequence"
        if self.inplace:
            freed = self.live()
            self.level[freed] = None
        else:
            freed = s
            self.level[s] = None
        if self.pending[wb] == 0:
            self.first_slot[wb] = freed
        else:
            assert (self.first_slot[wb] + self.pending[wb]) % self.D == freed, "freed slots of a window are not consecutive"
        self.pending[wb] += 1
        assert self.pending[wb] <= self.B + 1 < 256, "`pending` is a byte, and a window takes at most B + 1 of one env"
        self.next = (s + 1) % self.D
        if not self.parked:
            self.played += 1
            self.total_played += 1
        return self.pending[wb]

    def reseed(self, wb, k):
        assert not any(self.busy), "a reseed met a refill in flight"
        self.epoch += 1
        self._new_ring(k)
        self.pending[wb] = 0
        return self.finish(wb)

    def launch_refill(self, wb):
        jobs = []
        for j in range(self.pending[wb]):
            slot = (self.first_slot[wb] + j) % self.D
            assert not self.busy[slot], "two refills in flight for one slot"
            assert self.level[slot] is None, "the refill names a slot that is not free"
            self.busy[slot] = True
            jobs.append((slot, (self.epoch, self.gen_seq)))
            self.gen_seq += 1
        return jobs

    def land(self, jobs, wb):
        for slot, seq in jobs:
            assert self.busy[slot]
            assert self.level[slot] is None, "a refill landed on a slot that holds an unplayed level, a parking slot or a stale record nobody freed"
            assert seq[0] == self.epoch, "a refill of the old sequence landed behind a reseed"
            if self.inplace:
                assert slot != self.live() or self.total_played == 0, "a refill landed on the live slot"
            self.level[slot], self.busy[slot] = seq, False
        self.pending[wb] = 0


class Batch:
    """Several envs under ONE window clock, the gate of k_gate, refills that land in order, and reseeds with a depth."""

    def __init__(self, B, depth, inplace, n_envs, nwin=NWIN, rng=None, land_prob=0.0):
        self.B, self.nwin = B, nwin
        self.envs = [Env(B, depth, inplace, nwin) for _ in range(n_envs)]
        self.M = [0] * nwin
        self.in_flight = {}
        self.refilled = 0
        self.tick = 0
        self.rng, self.land_prob = rng, land_prob

    def land_one(self):
        w = self.refilled
        jobs = self.in_flight.pop(w)
        for e, j in zip(self.envs, jobs):
            e.land(j, w % self.nwin)
        self.refilled += 1

    def gate(self, x):
        while True:
            open_ = x - self.refilled
            if open_ < self.nwin and sum(max(1, self.M[v % self.nwin]) for v in range(self.refilled, x)) <= self.B:
                break
            assert self.refilled in self.in_flight, "the gate waits for a refill that was never launched"
            self.land_one()
        wb = x % self.nwin
        for e in self.envs:
            assert e.pending[wb] == e.early, "a window started on a buffer whose refill has not landed"
            e.early = 0
        self.M[wb] = 0

    def step(self, finished):
        w = self.tick // self.B
        if self.tick % self.B == 0:
            self.gate(w)
        wb = w % self.nwin
        for e, f in zip(self.envs, finished):
            if f and not e.parked:                       # (a parked env is frozen: the step does not move it)
                p = e.finish(wb)
                if p > 1:
                    self.M[wb] = max(self.M[wb], p)
        if self.tick % self.B == self.B - 1:
            self.in_flight[w] = [e.launch_refill(wb) for e in self.envs]
        self.tick += 1
        while self.rng is not None and self.refilled in self.in_flight and self.rng.rand() < self.land_prob:
            self.land_one()

    def reseed(self, i, k):
        while self.refilled in self.in_flight:
            self.land_one()
        w = self.tick // self.B
        wb = w % self.nwin
        e = self.envs[i]
        p = e.reseed(wb, k)
        if p > 1:
            self.M[wb] = max(self.M[wb], p)
        if self.tick % self.B == 0:
            e.early = e.pending[wb]


def _depth(B, inplace):
    return 2 * B + (1 if inplace else 0)


def _patterns(B, T, n, rng):
    ps = [1.0, 0.6, 0.03] + list(rng.choice([0.0, 0.3, 0.9], size=max(0, n - 3)))
    return rng.rand(T, n) < np.array(ps[:n])


def _depths(B):
    return [1, 2, 3, 2 * B - 1, 2 * B, 2 * B + 5]


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("B", [2, 4, 16])
@pytest.mark.parametrize("where", ["first", "last", "middle", "twice"])
def test_a_short_reseed_anywhere_in_a_window_keeps_every_invariant(B, inplace, where):
    n = 4
    rng = np.random.RandomState(100 * B + inplace)
    T = 12 * B
    fin = _patterns(B, T, n, rng)
    pos = {"first": [0], "last": [B - 1], "middle": [B // 2], "twice": [B // 2, B // 2] if B == 2 else [1, B - 1]}[where]
    for k in _depths(B):
        for target in range(3):                  # the env that finishes on every tick, the busy one, the quiet one
            b = Batch(B, _depth(B, inplace), inplace, n)
            was_parked = []
            for t in range(T):
                if t // B in (3, 4, 7) and t % B in pos:
                    for _ in range(pos.count(t % B)):
                        was_parked.append(b.envs[target].parked)
                        b.reseed(target, k)
                        assert not b.envs[target].parked                 # a reseed (any depth) brings a parked env back
                b.step(list(fin[t]))
            e = b.envs[target]
            assert e.epoch == 3 * len(pos)
            if k >= 2 * B:
                assert e.parkings == 0 and e.limit is None                # the whole ring: today's behaviour
            elif target == 0:                                             # finishes on every tick: spends k levels in k ticks
                assert e.parked and e.played == k
                if k <= B and where != "twice":
                    assert e.parkings == 3 and was_parked == [False, True, True]          # parked each time, and stayed parked until the next call
            for j, o in enumerate(b.envs):
                if j != target:
                    assert o.epoch == 0 and o.parkings == 0 and o.total_played == int(fin[:, j].sum())          # the others go on as if nothing had happened


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("B", [2, 4, 16])
def test_a_parked_env_stays_parked_and_its_slots_are_refilled_like_any_others(B, inplace):
    """Depth 1 in front of a window's first tick, a finish on every tick: the env parks on that tick, 2 slots booked; it is still parked 50
    windows later, the booked slots were refilled once (k + 1 levels nobody plays) and nothing else of its ring was touched."""
    b = Batch(B, _depth(B, inplace), inplace, 2)
    for t in range(2 * B):
        b.step([True, t % 3 == 0])
    b.reseed(0, 1)
    e = b.envs[0]
    ring = list(e.level)
    for t in range(50 * B):
        b.step([True, t % 3 == 0])
        if t == 0:
            assert e.parked and e.pending[2 % NWIN] == 2
    while b.refilled in b.in_flight:
        b.land_one()
    assert e.parked and e.played == 1 and e.gen_seq == 1 + 2
    assert sum(1 for s in range(e.D) if e.level[s] != ring[s]) == 2
    assert sum(1 for lv in e.level if lv == STALE) == sum(1 for lv in ring if lv == STALE) > 0
    assert b.envs[1].total_played == sum(1 for t in range(2 * B) if t % 3 == 0) + sum(1 for t in range(50 * B) if t % 3 == 0)


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("B", [2, 4, 16])
def test_short_reseeds_in_every_window_for_fifty_windows(B, inplace):
    n = 5
    rng = np.random.RandomState(7 * B + inplace)
    for land_prob in (0.0, 0.3):
        b = Batch(B, _depth(B, inplace), inplace, n, rng=rng if land_prob else None, land_prob=land_prob)
        T = 50 * B
        fin = _patterns(B, T, n, rng)
        ks = _depths(B) + [0]
        calls = 0
        for t in range(T):
            w = t // B
            if t % B == (w * 5) % B:                      # every window, at a position that walks through the window
                for i in ([w % n] if w % 4 else [w % n, (w + 2) % n]):
                    b.reseed(i, ks[(w + i) % len(ks)])
                    calls += 1
            if w % 7 == 3 and t % B == B - 1:             # ... and now and then a second call in the same window, same env
                b.reseed(w % n, ks[w % len(ks)])
                calls += 1
            b.step(list(fin[t]))
        assert sum(e.epoch for e in b.envs) == calls
        assert sum(e.parkings for e in b.envs) > 0


@pytest.mark.parametrize("inplace", [False, True])
def test_a_refill_that_named_the_parking_slot_would_be_caught(inplace):
    """Tightness of the model: were the parking slot booked for a refill before the env reached it (the generator overwriting the frozen state),
    the landing is refused."""
    B = 4
    b = Batch(B, _depth(B, inplace), inplace, 1)
    b.reseed(0, 2)
    e = b.envs[0]
    park = e.level.index(PARK)
    e.busy[park] = True
    with pytest.raises(AssertionError):
        e.land([(park, (e.epoch, 9))], 0)
