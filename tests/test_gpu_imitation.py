"""The demo store on the device: k_demo_spans vs `demos.scan_chunk`, `DemoStore.collect` vs `demos.generate_demos` (itself pinned to the
reference's script by test_gpu_parity.py::test_generate_demos_matches_reference_script), k_demo_batch vs the host path that
tests/test_imitation_host.py pins to the reference, and `run_batch` / `run_epoch` on the device vs the reference's recorded logs."""
import numpy as np
import pytest
import torch

import imitation_util as iu
from test_imitation_host import check_case, check_epoch, same_demos, spans_case, golden, vocab, CASES  # noqa: F401  (fixtures)

FIELDS = ("image", "action", "done", "mask", "episode_ids", "inds", "instr")


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 16, 128])
@pytest.mark.parametrize("n", [1, 63, 64, 200, 4099])
@pytest.mark.parametrize("filter_steps", [0, 3])
def test_span_kernel_equals_scan_chunk(gpu, chunk, n, filter_steps):
    for p_done in (0.02, 0.3):
        spans_case(np.random.default_rng(chunk * 7 + n), chunk, n, 4, filter_steps, p_done, device=gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("level,n,batch,filter_steps", [("GoToLocal", 300, 128, 0), ("GoToLocal", 100, 64, 6), ("PickupLoc", 200, 96, 0), ("GoTo", 150, 64, 0),
                                                        ("GoTo", 90, 40, 40), ("BossLevel", 100, 48, 0)])
def test_collect_equals_generate_demos(gpu, level, n, batch, filter_steps):
    from babyai_amd.demos import generate_demos
    from babyai_amd.imitation import DemoStore
    name = "BabyAI-%s-v0" % level
    ref = generate_demos(name, n, 77, device=gpu, batch=batch, filter_steps=filter_steps)
    store = DemoStore.collect(name, n, 77, device=gpu, batch=batch, filter_steps=filter_steps)
    assert len(store) == n and n % batch != 0 and store.image.is_cuda
    same_demos(store.to_reference(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("level,n,filter_steps", [("GoToLocal", 4096, 2), ("BossLevel", 512, 0)])
def test_collect_gathers_spans_from_later_chunks_and_across_chunk_boundaries(gpu, level, n, filter_steps):
    """k_demo_pack's chunk table: demos that begin in a later history chunk than the first, and demos whose frames lie in two chunks.
    A tight filter_steps makes streams pass many episodes before one is kept; BossLevel has episodes longer than a chunk.  Where the
    demos lie is computed (scan_chunk, the oracle of k_demo_spans, over the same rollout) and asserted, not assumed."""
    from babyai_amd.demos import generate_demos, scan_chunk
    from babyai_amd.engine import BatchedBabyAIEnv
    from babyai_amd.imitation import DemoStore
    name = "BabyAI-%s-v0" % level
    ref = generate_demos(name, n, 31, device=gpu, batch=n, filter_steps=filter_steps, rollout=True)
    store = DemoStore.collect(name, n, 31, device=gpu, batch=n, filter_steps=filter_steps)
    same_demos(store.to_reference(), ref)
    env = BatchedBabyAIEnv(name, n, device=gpu, seeds=[31 + k for k in range(n)], auto_reset=True)
    env.reset()
    chunk = max(1, min(128, max(16, env.max_steps_bound // 4)))             # as collect and generate_demos choose it
    last, open_, span, g0 = np.full(n, -1, np.int32), np.ones(n, bool), np.full((n, 2), -1, np.int64), 0
    while open_.any():
        r = env.bot_rollout(chunk)
        scan_chunk(r["done"].cpu().numpy(), r["gave_up"].cpu().numpy(), r["reward"].cpu().numpy(), g0, filter_steps, last, open_, span)
        g0 += chunk
    env.close()
    assert list(span[:, 1] - span[:, 0] + 1) == [len(d[3]) for d in ref]
    first, end = span[:, 0] // chunk, span[:, 1] // chunk
    print("chunk %d: %d chunks, demos beginning behind the first chunk %d, demos in two chunks %d" % (chunk, g0 // chunk, (first >= 1).sum(), (first != end).sum()))
    assert g0 // chunk >= 2 and (first != end).sum() >= 1, (chunk, g0)
    if filter_steps:
        assert (first >= 1).sum() >= 8


@pytest.mark.gpu
def test_collect_equals_generate_demos_in_done_action_mode(gpu, monkeypatch):
    from babyai_amd.demos import generate_demos
    from babyai_amd.imitation import DemoStore
    monkeypatch.setenv("BABYAI_DONE_ACTIONS", "1")
    ref = generate_demos("BabyAI-SynthSeq-v0", 60, 5, device=gpu, batch=32, rollout=True)
    store = DemoStore.collect("BabyAI-SynthSeq-v0", 60, 5, device=gpu, batch=32)
    same_demos(store.to_reference(), ref)
    assert any(" and " in d[0] for d in ref)
    # the mode really is on, and it matters: the expert ends its episodes with `done` actions, which the mode-off run never takes
    from babyai_amd.engine import BatchedBabyAIEnv
    env = BatchedBabyAIEnv("BabyAI-SynthSeq-v0", 4, device=gpu)
    assert env.done_actions
    env.close()
    monkeypatch.delenv("BABYAI_DONE_ACTIONS")
    off = DemoStore.collect("BabyAI-SynthSeq-v0", 60, 5, device=gpu, batch=32).to_reference()
    assert [list(d[3]) for d in off] != [list(d[3]) for d in ref]
    assert any(6 in d[3] for d in ref) and not any(6 in d[3] for d in off)


def host_copy(store):
    from babyai_amd.imitation import DemoStore
    return DemoStore(store.image.cpu(), store.direction.cpu(), store.action.cpu(), store.tokens.cpu(), store.offset_host)


def same_batch(a, b):
    assert list(a.order) == list(b.order) and list(a.lengths) == list(b.lengths)
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.is_cuda and x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y), f


@pytest.mark.gpu
def test_batch_kernel_equals_the_host_path(gpu):
    from babyai_amd.imitation import DemoStore
    store = DemoStore.collect("BabyAI-GoToLocal-v0", 160, 11, device=gpu, batch=160)
    host = host_copy(store)
    rng = np.random.default_rng(3)
    mixed = [int(i) for i in rng.permutation(160)[:96]]
    batch = store.batch(mixed)
    same_batch(batch, host.batch(mixed))
    src = {int(store.offset_host[k]) * 147 % 16 for k in batch.order}
    dst = {int(s) * 147 % 16 for s in batch.inds.cpu().tolist()}
    assert len(src) == 16 and len(dst) == 16, (sorted(src), sorted(dst))          # demos began at every byte phase on both sides
    same_batch(store.batch([7]), host.batch([7]))
    same_batch(store.batch(list(range(160))), host.batch(list(range(160))))
    twice = [5, 9, 5, 5, 160 - 1, 9]
    same_batch(store.batch(twice), host.batch(twice))
    same_batch(store.batch(torch.tensor(twice, device=gpu)), host.batch(twice))
    sub, hsub = store.select(mixed), host.select(mixed)
    assert sub.image.is_cuda
    for f in ("image", "direction", "action", "tokens", "offset"):
        assert torch.equal(getattr(sub, f).cpu(), getattr(hsub, f)), f


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_run_batch_on_the_device_equals_the_reference(gpu, golden, vocab, name):  # noqa: F811
    check_case(golden, vocab, name, gpu)


@pytest.mark.gpu
def test_run_epoch_on_the_device_equals_the_reference(gpu, golden, vocab):  # noqa: F811
    check_epoch(golden, vocab, gpu)
