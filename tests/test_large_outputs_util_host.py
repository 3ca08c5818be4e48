"""large_outputs_util on CPU tensors: the counts it gives, and that its comparisons fail where they must -- a checker that cannot fail
would make tests/test_gpu_large_outputs.py vacuous.  No GPU."""
import pytest

import large_outputs_util as lou

FRAMES = {"7x7 at 16": 37632, "7x7 at 32": 150528, "11x11 at 32 / BossLevel at 16": 371712, "3x3 at 8": 1728, "BossLevel at 32": 1486848,
          "BossLevel at 8": 92928}


def test_counts_cross_4_gib_with_a_frame_across_each_limit():
    for what, F in FRAMES.items():
        k = lou.count_for(F)
        assert (k - 3) * F >= (1 << 32) + (1 << 24) > (k - 4) * F, what
        j31, j32 = lou.straddlers(F)
        assert j31 * F < 1 << 31 < (j31 + 1) * F and j32 * F < 1 << 32 < (j32 + 1) * F and j32 + 1 < k - 3, what
        past = lou.first_frame_past(F)
        assert past == j32 + 1 and past * F >= 1 << 32 and k - past >= 3 + (1 << 24) // F, what
        rows = lou.slices(k, F)
        assert rows[0][0] == 0 and rows[-1][1] == k and all(a[1] == b[0] for a, b in zip(rows, rows[1:])), what
        assert all(0 < (hi - lo) * F <= max(F, lou.SLICE_BYTES) for lo, hi in rows), what
        assert any(lo * F < 1 << 32 < hi * F for lo, hi in rows) or any(lo * F == 1 << 32 for lo, hi in rows), what
    assert lou.count_for(150528) == 28648 and lou.count_for(1486848) == 2903
    assert [lou.where_of(o) for o in (0, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32)] == ["below 2^31"] * 2 + ["past 2^31"] * 2 + ["past 2^32"]


def test_rows_equal_passes_and_fails():
    import torch
    gen = torch.Generator().manual_seed(1)
    distinct = torch.randint(1, 256, (5, 4, 6, 3), dtype=torch.uint8, generator=gen)
    ids = torch.tensor([0, 4, 4, -1, 2, 5, 1 << 40, 3, 0], dtype=torch.int64)
    out = torch.zeros((9, 4, 6, 3), dtype=torch.uint8)
    for j, i in enumerate(ids.tolist()):
        if 0 <= i < 5:
            out[j] = distinct[i]
    assert lou.assert_rows_equal(out, distinct, ids) == 9 * 72 - 1
    assert lou.assert_rows_equal(out, distinct, ids) == lou.assert_same(out, out.clone())
    bad = out.clone()
    bad[7, 1, 2, 1] ^= 1                                # one bit of one byte
    with pytest.raises(AssertionError, match=r"row 7 differs from byte 25 .*byte offset %d in the output, below 2\^31" % (7 * 72 + 25)):
        lou.assert_rows_equal(bad, distinct, ids, "case")
    bad = out.clone()
    bad[3, 0, 0, 0] = 0xA5                              # a row of an id outside the batch must be zero
    with pytest.raises(AssertionError, match="row 3 differs from byte 0 "):
        lou.assert_rows_equal(bad, distinct, ids)
    bad = out.clone()
    bad[2] = distinct[3]                                # a whole frame of another env
    with pytest.raises(AssertionError, match="row 2 "):
        lou.assert_rows_equal(bad, distinct, ids)
    with pytest.raises(AssertionError, match="row 8 "):
        lou.assert_frames_equal(out, lambda lo, hi: torch.cat([out[lo:hi - 1], out[hi - 1:hi] + 1]) if hi == 9 else out[lo:hi])


def test_slices_split_a_comparison(monkeypatch):
    import torch
    monkeypatch.setattr(lou, "SLICE_BYTES", 100)
    assert lou.slices(7, 40, 100) == [(0, 2), (2, 4), (4, 6), (6, 7)] and lou.slices(3, 400, 100) == [(0, 1), (1, 2), (2, 3)]
    a = torch.arange(7 * 40, dtype=torch.int64).remainder(251).to(torch.uint8).view(7, 40)
    calls = []
    assert lou.assert_frames_equal(a, lambda lo, hi: calls.append((lo, hi)) or a[lo:hi].clone()) == 279
    assert calls == [(0, 2), (2, 4), (4, 6), (6, 7)]
    b = a.clone()
    b[6, 39] ^= 0x80
    with pytest.raises(AssertionError, match="row 6 differs from byte 39 .*byte offset 279"):
        lou.assert_same(a, b)


def test_banded_out_sees_a_write_on_either_side_and_an_unwritten_byte():
    import torch
    out, bands = lou.banded_out(3, (4, 5, 3), band=64, device="cpu")
    assert tuple(out.shape) == (3, 4, 5, 3) and out.data_ptr() % 16 == 0 and bool(out.eq(0xA5).all())
    bands()
    base = out.view(-1)
    storage = torch.tensor([], dtype=torch.uint8).set_(out.untyped_storage())
    off = out.storage_offset()
    assert off >= 64 and storage.numel() >= off + 180 + 64
    for pos in (off - 1, off + 180, 0, storage.numel() - 1):
        storage[pos] = 0
        with pytest.raises(AssertionError, match="in front of|behind"):
            bands()
        storage[pos] = 0xA5
        bands()
    base[:] = 7
    bands()
    base[100] = 0xA5                                    # a byte no render wrote: the poison shows
    with pytest.raises(AssertionError, match="row 1 differs from byte 40 "):
        lou.assert_same(out, torch.full_like(out, 7))
