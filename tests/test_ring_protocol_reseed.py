"""The look-ahead ring's window protocol with RESEEDS of single envs (bbai_reseed, babyai_amd/csrc/bbai_reseedk.hpp; the rule at NWIN in
bbai_kernels.hpp), as a model: host logic, no GPU.  The model of tests/test_ring_protocol.py (its own copy here) plus
one event.  A reseed of env i

  * waits for every refill launched so far (the call's first look-ahead stream stands behind all of them),
  * replaces the env's whole ring by levels 0 .. fill - 1 of a NEW sequence (fill = D, or D - 1 in place: the empty live slot D - 1),
  * clears the env's byte in the CURRENT window's buffer (what the env consumed there before needs no refill any more), and
  * consumes slot 0, booked into the current window like any finished env's reset: pending 1, the freed slot first.

It is no consume-tick.  With it ONE env can consume B + 1 slots in one window (a reseed in front of the window's first tick, then a finish
on every tick): M records that through the consume paths' atomicMax, and the gate then holds the next window until this window's refill has
landed -- the ring is freshly full, so B + 1 <= 2B slots are there.  Checked: every invariant of the original model, an env always finds
the next level of its CURRENT sequence, under refills that land as late as the gate allows; and a reseed that leaves the current buffer's
byte as it was, or books no consumption, breaks an invariant (both parts of the rule are needed).
"""
import numpy as np
import pytest

NWIN = 34            # bbai_kernels.hpp NWIN


class Env:
    """One env's ring under the engine's bookkeeping; a level is (sequence it belongs to, number in it)."""

    def __init__(self, B, depth, inplace, nwin):
        self.B, self.D, self.inplace = B, depth, inplace
        self.fill = depth - 1 if inplace else depth      # bbai_seed / k_reseed_seed: pending = depth - inplace levels from slot 0
        self.epoch = 0
        self.busy = [False] * depth          # a refill for this slot has been launched and has not landed yet
        self.pending = [0] * nwin
        self.first_slot = [0] * nwin
        self.early = 0                       # booked by reseeds into a window whose gate has not run yet
        self.total_played = 0
        self._new_ring()

    def _new_ring(self):
        self.level = [(self.epoch, s) if s < self.fill else None for s in range(self.D)]
        self.gen_seq = self.fill             # next number the generator produces for this env
        self.next = 0                        # hot.slot
        self.played = 0                      # number of the next level of the current sequence the env must get

    def live(self):
        return (self.next - 1) % self.D

    def finish(self, wb, book=True):
        s = self.next
        assert not self.busy[s], "the env moved to a slot whose refill has not landed"
        assert self.level[s] == (self.epoch, self.played), "the env did not get the next level of its current sequence"
        if self.inplace:
            freed = self.live()
            self.level[freed] = None
        else:
            freed = s
            self.level[s] = None
        if book:
            if self.pending[wb] == 0:
                self.first_slot[wb] = freed
            else:
                assert (self.first_slot[wb] + self.pending[wb]) % self.D == freed, "freed slots of a window are not consecutive"
            self.pending[wb] += 1
        self.next = (s + 1) % self.D
        self.played += 1
        self.total_played += 1
        return self.pending[wb]

    def reseed(self, wb, clear=True, book=True):
        assert not any(self.busy), "a reseed met a refill in flight"          # (the call stands behind every launched refill)
        self.epoch += 1
        self._new_ring()
        if clear:
            self.pending[wb] = 0
        return self.finish(wb, book)

    def launch_refill(self, wb):
        jobs = []
        for k in range(self.pending[wb]):
            slot = (self.first_slot[wb] + k) % self.D
            assert not self.busy[slot], "two refills in flight for one slot"
            assert self.level[slot] is None, "the refill names a slot that is not free"
            self.busy[slot] = True
            jobs.append((slot, (self.epoch, self.gen_seq)))
            self.gen_seq += 1
        return jobs

    def land(self, jobs, wb):
        for slot, seq in jobs:
            assert self.busy[slot]
            assert self.level[slot] is None, "a refill landed on a slot that still holds a level"
            assert seq[0] == self.epoch, "a refill of the old sequence landed behind a reseed"
            if self.inplace:
                assert slot != self.live() or self.total_played == 0, "a refill landed on the live slot"
            self.level[slot], self.busy[slot] = seq, False
        self.pending[wb] = 0


class Batch:
    """Several envs under ONE window clock, the gate of k_gate, refills that land in order, and reseeds."""

    def __init__(self, B, depth, inplace, n_envs, nwin=NWIN, rng=None, land_prob=0.0):
        self.B, self.nwin = B, nwin
        self.envs = [Env(B, depth, inplace, nwin) for _ in range(n_envs)]
        self.M = [0] * nwin
        self.in_flight = {}
        self.refilled = 0
        self.tick = 0
        self.rng, self.land_prob = rng, land_prob
        self.max_M = 0

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
            if f:
                p = e.finish(wb)
                if p > 1:
                    self.M[wb] = max(self.M[wb], p)
        self.max_M = max(self.max_M, self.M[wb])
        if self.tick % self.B == self.B - 1:
            self.in_flight[w] = [e.launch_refill(wb) for e in self.envs]
        self.tick += 1
        while self.rng is not None and self.refilled in self.in_flight and self.rng.rand() < self.land_prob:
            self.land_one()

    def reseed(self, i, clear=True, book=True):
        """bbai_reseed of env i in front of tick `self.tick`: no consume-tick, no gate, no refill launch."""
        while self.refilled in self.in_flight:          # every refill launched so far has landed before the env's ring is touched
            self.land_one()
        w = self.tick // self.B                         # the current window (at its first tick: the one about to open)
        wb = w % self.nwin
        e = self.envs[i]
        p = e.reseed(wb, clear, book)
        if p > 1:
            self.M[wb] = max(self.M[wb], p)
        if self.tick % self.B == 0:                     # its gate is still to come: it finds the byte this call booked
            e.early = e.pending[wb]


def _depth(B, inplace):
    return 2 * B + (1 if inplace else 0)


def _patterns(B, T, n, rng):
    """env 0 finishes on every tick (the worst case), env 1 often, env 2 rarely, the rest at random rates"""
    ps = [1.0, 0.6, 0.03] + list(rng.choice([0.0, 0.3, 0.9], size=max(0, n - 3)))
    return rng.rand(T, n) < np.array(ps[:n])


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("B", [2, 4, 16])
@pytest.mark.parametrize("where", ["first", "last", "middle", "twice"])
def test_a_reseed_anywhere_in_a_window_keeps_every_invariant(B, inplace, where):
    n = 4
    rng = np.random.RandomState(100 * B + inplace)
    T = 12 * B
    fin = _patterns(B, T, n, rng)
    pos = {"first": [0], "last": [B - 1], "middle": [B // 2], "twice": [B // 2, B // 2] if B == 2 else [1, B - 1]}[where]
    for target in range(3):                  # the env that finishes on every tick, the busy one, the quiet one
        b = Batch(B, _depth(B, inplace), inplace, n)
        for t in range(T):
            if t // B in (3, 4, 7) and t % B in pos:
                for _ in range(pos.count(t % B)):
                    b.reseed(target)
            b.step(list(fin[t]))
        e = b.envs[target]
        assert e.epoch == 3 * len(pos)
        assert e.total_played == int(fin[:, target].sum()) + e.epoch
        for k, o in enumerate(b.envs):
            if k != target:
                assert o.epoch == 0 and o.total_played == int(fin[:, k].sum())          # the others go on as if nothing had happened


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("B", [2, 4, 16])
def test_b_plus_one_slots_in_one_window(B, inplace):
    """A reseed in front of a window's first tick, then a finish on every tick: B + 1 consumptions of one env in one window.  M says so,
    the gate holds the next window until this one's refill has landed, and the freshly filled ring has the levels."""
    b = Batch(B, _depth(B, inplace), inplace, 2)
    for t in range(6 * B):
        if t == 2 * B:
            b.reseed(0)
        b.step([True, t % 3 == 0])
        if t == 3 * B - 1:
            assert b.envs[0].pending[2 % NWIN] == B + 1 and b.M[2 % NWIN] == B + 1
        if t == 3 * B:
            assert b.refilled == 3, "the gate behind a window with M = B + 1 waits for that window's refill"
    assert b.max_M == B + 1


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("B", [2, 4, 16])
def test_reseeds_in_every_window_for_fifty_windows(B, inplace):
    n = 5
    rng = np.random.RandomState(7 * B + inplace)
    for land_prob in (0.0, 0.3):
        b = Batch(B, _depth(B, inplace), inplace, n, rng=rng if land_prob else None, land_prob=land_prob)
        T = 50 * B
        fin = _patterns(B, T, n, rng)
        calls = 0
        for t in range(T):
            w = t // B
            if t % B == (w * 5) % B:                      # every window, at a position that walks through the window
                for i in ([w % n] if w % 4 else [w % n, (w + 2) % n]):
                    b.reseed(i)
                    calls += 1
            if w % 7 == 3 and t % B == B - 1:             # ... and now and then a second call in the same window, same env
                b.reseed(w % n)
                calls += 1
            b.step(list(fin[t]))
        assert sum(e.epoch for e in b.envs) == calls
        assert sum(e.total_played for e in b.envs) == int(fin.sum()) + calls


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("B", [2, 4, 16])
def test_the_current_windows_byte_must_be_cleared(B, inplace):
    """Tightness: the env consumed in this window before the call; with its byte left standing the window's refill names slots that the
    reseed has just filled (or the booking is no longer a run of consecutive slots)."""
    with pytest.raises(AssertionError):
        b = Batch(B, _depth(B, inplace), inplace, 1)
        for t in range(4 * B):
            if t == 2 * B + B - 1:
                b.reseed(0, clear=False)
            b.step([True])


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("B", [2, 4, 16])
def test_the_reseeds_consumption_must_be_booked(B, inplace):
    """Tightness: a reseed that books nothing leaves the slot it freed without a refill -- a ring's turn later the env finds no level there."""
    with pytest.raises(AssertionError):
        b = Batch(B, _depth(B, inplace), inplace, 1)
        for t in range(8 * B + 4):
            if t == 2 * B + 1:
                b.reseed(0, book=False)
            b.step([True])
