"""Helpers of the GPU tests whose outputs cross the 2 GiB and 4 GiB byte offsets (tests/test_gpu_large_outputs.py): the smallest frame
counts that do, an output buffer with poisoned body and guard bands, and a row-by-row comparison that stays on the device and never
indexes more than 256 MiB itself -- so a 32-bit product in a kernel, a launch record, a planner or the binding shows as wrong or missing
bytes, and the checker's own arithmetic cannot.  Plain Python and torch.  Test harness only."""

LIMIT_2G, LIMIT_4G = 1 << 31, 1 << 32
SLICE_BYTES = 256 << 20
BAND, BAND_BYTE = 4096, 0xA5


def count_for(frame_bytes):
    """The smallest k with k * frame_bytes >= 2^32 + 2^24, plus 3: the output ends 16 MiB or more past 4 GiB, one frame lies across 2^31
    and one across 2^32 (straddlers), and for the frame sizes in use the count leaves a partial last launch group -- but for the 7x7
    view at 32, 28 648 frames = 3 581 groups of k_view_delta's 8 (the callers assert what holds for them)."""
    return -(-(LIMIT_4G + (1 << 24)) // int(frame_bytes)) + 3


def straddlers(frame_bytes):
    """(j31, j32): the frames that hold byte offsets 2^31 and 2^32 of a buffer of such frames (asserted to lie across them, not to start
    there)."""
    F = int(frame_bytes)
    out = []
    for limit in (LIMIT_2G, LIMIT_4G):
        j = limit // F
        assert j * F < limit < (j + 1) * F, (F, limit)
        out.append(j)
    return tuple(out)


def first_frame_past(frame_bytes, limit=LIMIT_4G):
    """The first frame that lies wholly at or beyond byte offset `limit`."""
    return -(-limit // int(frame_bytes))


def need_memory(nbytes, device=None):
    """Fails (not skips, like the `gpu` fixture) where the device has less free memory than the case allocates."""
    import pytest
    import torch
    free, total = torch.cuda.mem_get_info(device)
    if free < nbytes:
        pytest.fail("this case allocates %.1f GB on the device, which has %.1f GB free of %.1f GB" % (nbytes / 1e9, free / 1e9, total / 1e9))


def banded_out(k, shape, band=BAND, byte=BAND_BYTE, device="cuda:0"):
    """One flat uint8 allocation filled with `byte`: a band, the [k, *shape] frames on a 16-byte boundary, a band.  Returns (frames,
    check); check() asserts that every byte of both bands still holds `byte`.  The body is poisoned as well: a byte of a frame that a
    render never wrote still holds `byte` and fails the comparison with the expected frame."""
    import torch
    F = 1
    for s in shape:
        F *= int(s)
    raw = torch.full((band + k * F + band + 16,), byte, dtype=torch.uint8, device=device)
    lo = band + (-(raw.data_ptr() + band)) % 16
    frames = raw[lo:lo + k * F].view((k,) + tuple(int(s) for s in shape))
    assert frames.data_ptr() % 16 == 0 and frames.data_ptr() == raw.data_ptr() + lo and frames.is_contiguous()

    def check():
        front, back = raw[:lo], raw[lo + k * F:]
        assert front.numel() >= band and back.numel() >= band
        assert bool(front.eq(byte).all()), "bytes in front of the output were written"
        assert bool(back.eq(byte).all()), "bytes behind the output were written"
    return frames, check


def where_of(offset):
    return "past 2^32" if offset >= LIMIT_4G else "past 2^31" if offset >= LIMIT_2G else "below 2^31"


def slices(k, frame_bytes, limit=None):
    """[lo, hi) row ranges of at most `limit` bytes each (SLICE_BYTES; one row where a row is larger) that cover k rows."""
    rows = max(1, (SLICE_BYTES if limit is None else limit) // int(frame_bytes))
    return [(lo, min(k, lo + rows)) for lo in range(0, k, rows)]


def _report(got, want, lo, F, what):
    """AssertionError text for the first row of got[...] != want[...], rows counted from `lo`."""
    ne = (got != want).reshape(got.shape[0], -1)
    row = int(ne.any(dim=1).nonzero()[0])
    first = int(ne[row].nonzero()[0])
    off = (lo + row) * F + first
    return "%s: row %d differs from byte %d on (%d wrong bytes in the row): byte offset %d in the output, %s; got %s, want %s" % (
        what, lo + row, first, int(ne[row].sum()), off, where_of(off), got.reshape(got.shape[0], -1)[row, first:first + 8].tolist(),
        want.reshape(want.shape[0], -1)[row, first:first + 8].tolist())


def assert_rows_equal(out, distinct, ids, what=""):
    """out[j] == distinct[ids[j]] for every j -- all zeros where ids[j] lies outside [0, len(distinct)).  `ids`: int64[k] on the device.
    Compared on the device in slices of at most 256 MiB; returns the highest byte offset verified."""
    import torch
    k, m = int(out.shape[0]), int(distinct.shape[0])
    assert tuple(out.shape[1:]) == tuple(distinct.shape[1:]) and int(ids.shape[0]) == k and ids.dtype == torch.int64
    F = out[0].numel() * out.element_size()
    for lo, hi in slices(k, F):
        idx = ids[lo:hi]
        outside = (idx < 0) | (idx >= m)
        want = distinct[idx.clamp(0, m - 1)]
        want[outside] = 0
        got = out[lo:hi]
        if not torch.equal(got, want):
            raise AssertionError(_report(got, want, lo, F, what))
        del want
    return k * F - 1


def assert_frames_equal(out, expected, what=""):
    """out[lo:hi] == expected(lo, hi) for the slices of at most 256 MiB that cover `out`; `expected` builds its rows on the device.
    Returns the highest byte offset verified."""
    import torch
    k = int(out.shape[0])
    F = out[0].numel() * out.element_size()
    for lo, hi in slices(k, F):
        want = expected(lo, hi)
        got = out[lo:hi]
        assert tuple(want.shape) == tuple(got.shape), (what, tuple(want.shape), tuple(got.shape))
        if not torch.equal(got, want):
            raise AssertionError(_report(got, want, lo, F, what))
        del want
    return k * F - 1


def assert_same(a, b, what=""):
    """Two equally shaped device tensors hold the same bytes, compared in slices of at most 256 MiB."""
    assert tuple(a.shape) == tuple(b.shape), (what, tuple(a.shape), tuple(b.shape))
    return assert_frames_equal(a, lambda lo, hi: b[lo:hi], what)
