"""babyai_amd.imitation on host tensors vs the reference's own `transform_demos` + `ImitationLearning.run_epoch_recurrence_one_batch`
(babyai/imitation.py:189-321), run UNMODIFIED over tests/imitation_util.ToyILModel by tools/gen_golden_imitation.py: every integer
array, every model call's inputs, the logs and the parameters after one SGD step must be reproduced exactly.  Plus the store's
round trips and the span scan's host path against `demos.scan_chunk`."""
import json
import os

import numpy as np
import pytest
import torch
from hypothesis import given, settings, strategies as st

import imitation_util as iu
from babyai_amd import missions
from babyai_amd.demos import scan_chunk
from babyai_amd.imitation import DemoStore, demo_spans, run_batch, run_epoch

CASES = ("stable", "tail", "one")


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(iu.GOLDEN, "cases.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def vocab():
    with open(os.path.join(iu.GOLDEN, "vocab.json")) as f:
        return json.load(f)


def check_case(golden, vocab, name, device):
    g = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}
    store = DemoStore.from_reference(iu.load_demos(str(g["level"])), device=device)
    batch = store.batch([int(i) for i in g["indices"]], vocab=vocab)
    assert list(batch.order) == list(g["order"]) and list(batch.lengths) == list(g["lengths"])
    for field, ref in (("inds", g["inds"]), ("mask", g["mask"].reshape(-1, 1)), ("episode_ids", g["episode_ids"]), ("action", g["action_true"])):
        got = getattr(batch, field).cpu()
        assert got.dtype == {"mask": torch.float32}.get(field, torch.int64), field
        assert np.array_equal(got.numpy(), ref), (name, field)
    done = np.zeros(batch.num_frames, bool)
    done[np.cumsum(g["lengths"]) - 1] = True
    assert batch.done.dtype == torch.bool and np.array_equal(batch.done.cpu().numpy(), done)
    model = iu.ToyILModel().to(device)
    model.calls = []
    log = run_batch(model, batch, int(g["recurrence"]), iu.ENTROPY_COEF, optimizer=torch.optim.SGD(model.parameters(), lr=iu.LR))
    assert len(model.calls) == int(g["num_calls"])
    for c, call in enumerate(model.calls):
        for k in ("image", "memory", "emb"):
            ref = g["call%d/%s" % (c, k)]
            assert call[k].shape == ref.shape and np.array_equal(call[k], ref), (name, c, k)
        assert iu.strip(call["instr"]) == iu.strip(g["call%d/instr" % c]), (name, c)
    assert [log["entropy"], log["policy_loss"], log["accuracy"]] == list(g["log"]), (name, log)        # bit for bit
    assert np.array_equal(model.weight.detach().cpu().numpy(), g["weight_after"]), name


@pytest.mark.parametrize("name", CASES)
def test_batch_and_run_batch_equal_the_reference(golden, vocab, name):
    check_case(golden, vocab, name, "cpu")


def test_cases_cover_what_they_are_meant_to(golden):
    lens = list(golden["stable/lengths"])
    assert len(set(lens)) < len(lens) and len(set(golden["stable/indices"])) < len(golden["stable/indices"])      # ties, a repeated demo
    assert list(golden["stable/order"]) != list(golden["stable/indices"])                                          # the sort moved something
    F, r = int(golden["tail/lengths"].sum()), int(golden["tail/recurrence"])
    assert F % r != 0 and r > 1                                                                                  # starting_indexes drops a tail
    assert len(golden["one/lengths"]) == 1


def check_epoch(golden, vocab, device):
    store = DemoStore.from_reference(iu.load_demos(str(golden["epoch/level"])), device=device)
    model = iu.ToyILModel().to(device)
    log = run_epoch(model, store, [int(i) for i in golden["epoch/indices"]], 4, 1, iu.ENTROPY_COEF, vocab=vocab)
    assert model.training
    for k in ("entropy", "policy_loss", "accuracy"):
        assert log[k] == list(golden["epoch/" + k]), (k, log[k])
    assert log["total_frames"] == int(golden["epoch/total_frames"])


def test_run_epoch_equals_the_reference(golden, vocab):
    check_epoch(golden, vocab, "cpu")


def test_starting_indexes(golden):
    store = DemoStore.from_reference(iu.load_demos(iu.LEVELS[1]))
    batch = store.batch(list(range(len(store))))
    F = batch.num_frames
    for r in (1, 2, 3, 4, 5, 7, F):
        ref = np.arange(0, F, r) if F % r == 0 else np.arange(0, F, r)[:-1]
        assert np.array_equal(batch.starting_indexes(r).numpy(), ref)
    for t in range(int(batch.lengths[0])):
        ref = [int(batch.inds[b]) + t for b in range(len(batch)) if batch.lengths[b] > t]
        assert batch.active(t).tolist() == ref


def same_demos(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[0] == y[0] and list(x[2]) == list(y[2]) and list(x[3]) == list(y[3])
        assert np.asarray(x[1]).dtype == np.uint8 and np.array_equal(x[1], y[1])


def test_reference_round_trip_plain_and_packed():
    from oracle import refenv
    refenv.enable_shim()
    import blosc
    for level in iu.LEVELS:
        demos = iu.load_demos(level)
        store = DemoStore.from_reference(demos)
        assert len(store) == len(demos) and store.num_frames == sum(len(d[3]) for d in demos)
        same_demos(store.to_reference(), demos)
        packed = [(d[0], blosc.pack_array(d[1]), d[2], d[3]) for d in demos]
        again = DemoStore.from_reference(packed, unpack=blosc.unpack_array).to_reference(pack=blosc.pack_array)
        same_demos([(d[0], blosc.unpack_array(d[1]), d[2], d[3]) for d in again], demos)
        for k, d in enumerate(demos):
            ids = missions.tokenize(d[0])
            assert store.tokens[k, :len(ids)].tolist() == ids and not store.tokens[k, len(ids):].any()


def test_save_load_select_and_index_tensors(tmp_path):
    demos = iu.load_demos(iu.LEVELS[1])
    store = DemoStore.from_reference(demos)
    path = str(tmp_path / "store.npz")
    store.save(path)
    same_demos(DemoStore.load(path).to_reference(), demos)
    pick = [5, 0, 11, 5, 3]
    sub = store.select(pick)
    same_demos(sub.to_reference(), [demos[i] for i in pick])
    same_demos(store.select(torch.tensor(pick)).to_reference(), [demos[i] for i in pick])
    assert len(store.select([])) == 0
    a, b = store.batch(pick), store.batch(torch.tensor(pick))
    for f in ("image", "action", "done", "mask", "episode_ids", "inds", "instr"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    # the batch of a selection = the batch of the same demos of the whole store
    c = sub.batch(list(range(len(pick))))
    for f in ("image", "action", "done", "mask", "episode_ids", "inds", "instr"):
        assert torch.equal(getattr(a, f), getattr(c, f)), f
    with pytest.raises(IndexError):
        store.batch([len(store)])


def spans_case(rng, chunk, n, chunks, filter_steps, p_done, device="cpu"):
    """A few chunks in a row through the carry, against scan_chunk.  Returns what both ended with."""
    last_ref, open_ref, span_ref = np.full(n, -1, np.int32), np.ones(n, bool), np.full((n, 2), -1, np.int64)
    last = torch.full((n,), -1, dtype=torch.int32, device=device)
    open_ = torch.ones(n, dtype=torch.uint8, device=device)
    span = torch.full((n, 2), -1, dtype=torch.int32, device=device)
    for c in range(chunks):
        done = (rng.random((chunk, n)) < p_done).astype(np.uint8)
        done[0, : n // 3] |= rng.random(n // 3) < 0.5                          # episodes that end on a chunk's first row ...
        done[-1, n // 3: 2 * (n // 3)] |= rng.random(n // 3) < 0.5             # ... and on its last
        if n > 2:
            done[:, -1] = 0                                                    # a stream that never closes
        gave_up = (rng.random((chunk, n)) < 0.2).astype(np.uint8)
        reward = np.where(rng.random((chunk, n)) < 0.5, rng.random((chunk, n)), 0).astype(np.float32)
        scan_chunk(done, gave_up, reward, c * chunk, filter_steps, last_ref, open_ref, span_ref)
        left = demo_spans(torch.as_tensor(done, device=device), torch.as_tensor(gave_up, device=device), torch.as_tensor(reward, device=device),
                          c * chunk, filter_steps, last, open_, span)
        assert int(left.cpu().reshape(-1)[0]) == int(open_ref.sum()), (c, chunk, n)
        assert np.array_equal(last.cpu().numpy(), last_ref), c
        assert np.array_equal(open_.cpu().numpy().astype(bool), open_ref), c
        assert np.array_equal(span.cpu().numpy().astype(np.int64), span_ref), c
    return open_ref


@settings(max_examples=30, deadline=None)
@given(seed=st.integers(0, 2 ** 31 - 1), chunk=st.sampled_from([1, 16, 128]), n=st.integers(1, 200), filter_steps=st.sampled_from([0, 1, 3, 9]),
       p_done=st.sampled_from([0.02, 0.2, 0.7]))
def test_span_scan_equals_scan_chunk(seed, chunk, n, filter_steps, p_done):
    spans_case(np.random.default_rng(seed), chunk, n, 4, filter_steps, p_done)


def test_span_scan_streams_that_never_close():
    still = spans_case(np.random.default_rng(7), 16, 64, 3, 2, 0.3)
    assert still[-1] and not still.all()
