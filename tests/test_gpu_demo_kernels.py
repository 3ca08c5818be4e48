"""k_demo_pack and k_demo_batch (babyai_amd/csrc/bbai_demo.hpp) on synthetic shapes that no rollout produces: one-frame demos that fill
a block's run table, chunk_steps of 1 and 3, demos longer than a block, every tail residue, selections of one demo, and the entries'
argument checks.  The inputs are seeded random bytes that go straight through the C ABI on the current stream; the references are the
plain numpy loops of tests/imitation_util.py (the batch one is pinned here, without a GPU, to the host path of `imitation._gather`, which
tests/test_imitation_host.py pins to the reference).  Every output sits at the front of a buffer filled with 0xA5 whose bytes behind the
output must stay as they were; equality is exact.  No env is created in this file."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import imitation_util as iu

ROW = iu.ROW
GUARD = 256                     # bytes behind every output (at least 64), and they keep the fill
FILL = 0xA5
BBAI_ERR_ARG = -1               # include/bbai.h


class Guarded(object):
    """`nbytes` of output at the front of a larger device buffer filled with FILL."""

    def __init__(self, nbytes, device):
        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + GUARD,), FILL, dtype=torch.uint8, device=device)
        assert GUARD >= 64 and self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr()

    def result(self, dtype, *shape):
        host = self.buf.cpu().numpy()
        assert host.size == self.nbytes + GUARD and (host[self.nbytes:] == FILL).all(), "bytes behind the output were written"
        return host[:self.nbytes].view(dtype).reshape(shape)

    def untouched(self):
        return bool((self.buf.cpu().numpy() == FILL).all())


def current_stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def upload(array, device):
    """One torch allocation per array: it starts 16-byte aligned (asserted) in a block that the caching allocator pads to 512 bytes,
    which is what the kernels' aligned 16-byte fetches around the source bytes need (include/bbai.h)."""
    t = torch.as_tensor(np.ascontiguousarray(array), device=device)
    assert t.is_contiguous() and t.data_ptr() % 16 == 0
    return t


# ------------------------------------------------------------------------------------------
# k_demo_pack
# ------------------------------------------------------------------------------------------
PACK_ARGS = ("n", "frames", "chunk_steps", "chunks", "span", "offset", "image", "direction", "action", "tokens")


def pack_setup(device, case):
    """The arguments of bbai_demo_pack for a case, by name; the guarded outputs; and the device tensors that must outlive the call."""
    hist = [{k: upload(h[k], device) for k in iu.HIST_KEYS} for h in case.hist]
    keep = {"hist": hist, "span": upload(case.span, device), "offset": upload(case.offset, device),
            "table": upload(np.array([[h[k].data_ptr() for k in iu.HIST_KEYS] for h in hist], dtype=np.int64), device)}
    outs = {"image": Guarded(case.frames * ROW, device), "direction": Guarded(case.frames, device), "action": Guarded(case.frames, device),
            "tokens": Guarded(case.n * iu.TOK_MAX, device)}
    args = {"n": case.n, "frames": case.frames, "chunk_steps": case.T, "chunks": keep["table"].data_ptr(), "span": keep["span"].data_ptr(),
            "offset": keep["offset"].data_ptr()}
    args.update({k: o.ptr for k, o in outs.items()})
    return args, outs, keep


def call_pack(device, args):
    from babyai_amd.engine import load_library
    lib = load_library()
    with torch.cuda.device(device):
        return lib, lib.bbai_demo_pack(*[args[k] for k in PACK_ARGS], current_stream(device))


def check_pack(device, case):
    from babyai_amd.engine import _check
    assert case.span.dtype == np.int32 and case.offset.dtype == np.int64 and len(case.hist) == case.C
    args, outs, keep = pack_setup(device, case)
    lib, rc = call_pack(device, args)
    _check(lib, rc, "bbai_demo_pack")
    torch.cuda.current_stream(device).synchronize()
    got = {"image": outs["image"].result(np.uint8, case.frames, ROW), "direction": outs["direction"].result(np.uint8, case.frames),
           "action": outs["action"].result(np.uint8, case.frames), "tokens": outs["tokens"].result(np.uint8, case.n, iu.TOK_MAX)}
    for k in iu.HIST_KEYS:
        assert np.array_equal(got[k], case.expect[k]), (k, np.flatnonzero((got[k] != case.expect[k]).reshape(len(got[k]), -1).any(axis=1))[:8])
    del keep


@pytest.mark.gpu
def test_pack_one_frame_demos_fill_a_blocks_run_table(gpu):
    """300 demos of one frame: every 8 KiB block meets 56 or 57 runs, so demo_find_lds lands near the top of the 64-entry slice."""
    rng = np.random.default_rng(101)
    case = iu.PackCase(rng, T=16, C=4, n=300, lens=np.ones(300, np.int64))
    assert (case.span[:, 0] == case.span[:, 1]).all() and case.frames == 300
    assert max(iu.runs_per_block(case.offset)) >= 56, iu.runs_per_block(case.offset)
    assert len(set(case.span[:, 0] // 16)) == 4                                # every chunk of the table is read
    check_pack(gpu, case)


@pytest.mark.gpu
def test_pack_chunk_steps_of_one(gpu):
    """T = 1: every frame of a demo lies in another chunk of the table."""
    rng = np.random.default_rng(102)
    lens = rng.integers(1, 41, size=65)
    lens[:3] = (1, 40, 2)
    case = iu.PackCase(rng, T=1, C=48, n=65, lens=lens)
    assert lens.min() == 1 and lens.max() == 40
    assert case.chunks_spanned.max() >= 3
    assert (case.chunks_spanned[lens > 1] > 1).all() and (case.chunks_spanned == lens).all()
    check_pack(gpu, case)


@pytest.mark.gpu
def test_pack_demos_longer_than_a_block(gpu):
    """T = 3 and three demos of 200 to 290 frames among short ones: blocks that begin deep inside a run (strongly negative s_rel[0]), blocks
    wholly inside one demo, demos in many chunks."""
    rng = np.random.default_rng(103)
    lens = rng.choice([1, 2, 5, 17], size=130)
    where = rng.choice(130, size=3, replace=False)
    lens[where] = (200, 247, 290)
    case = iu.PackCase(rng, T=3, C=100, n=130, lens=lens)
    assert sorted(lens[where]) == [200, 247, 290] and set(np.delete(lens, where)) == {1, 2, 5, 17}
    assert iu.blocks_inside_one_run(case.offset) >= 1
    assert case.chunks_spanned.max() >= 200 // 3
    check_pack(gpu, case)


# (n, lengths): the store's frame count takes every residue modulo 4 (the scalar branch of the direction / action writes at 1, 2, 3) and, as
# frames * 147 % 16, many lengths of the image array's last, byte-wise stored chunk
PACK_TAILS = [(1, (1,)), (1, (2,)), (1, (3,)), (1, (5,)), (7, (1, 1, 1, 1, 1, 1, 1)), (7, (1, 1, 1, 1, 1, 1, 2)), (7, (1, 2, 1, 1, 2, 1, 1)),
              (7, (3, 1, 1, 1, 2, 1, 1)), (7, (1, 1, 4, 1, 1, 3, 2)), (7, (5, 1, 3, 1, 2, 1, 1)), (7, (2, 2, 2, 2, 2, 2, 4))]


@pytest.mark.gpu
@pytest.mark.parametrize("n,lens", PACK_TAILS, ids=["n%d_f%d" % (n, sum(l)) for n, l in PACK_TAILS])
def test_pack_tails(gpu, n, lens):
    seven = [sum(l) for m, l in PACK_TAILS if m == 7]
    assert [sum(l) for m, l in PACK_TAILS if m == 1] == [1, 2, 3, 5] and {f % 4 for f in seven} == {0, 1, 2, 3}
    residues = {sum(l) * ROW % 16 for _, l in PACK_TAILS}
    assert len(residues - {0}) >= 8, sorted(residues)
    case = iu.PackCase(np.random.default_rng(104 + sum(lens)), T=4, C=3, n=n, lens=np.array(lens))
    assert case.frames == sum(lens) and case.n == n
    check_pack(gpu, case)


@pytest.mark.gpu
def test_pack_many_streams(gpu):
    """n = 4099: several blocks of direction / action lanes, many blocks of token lanes and a partial last one."""
    rng = np.random.default_rng(105)
    lens = rng.integers(1, 13, size=4099)
    case = iu.PackCase(rng, T=16, C=4, n=4099, lens=lens)
    assert set(lens) == set(range(1, 13))
    assert ((case.frames + 3) // 4 + 255) // 256 >= 3                          # meta blocks
    assert 4099 * 9 // 256 >= 100 and 4099 * 9 % 256 != 0                      # token blocks, the last one partial
    assert case.chunks_spanned.max() == 2 and len(set(case.span[:, 0] // 16)) == 4
    check_pack(gpu, case)


@pytest.mark.gpu
def test_pack_spans_at_the_ends_of_the_history(gpu):
    T, C = 5, 6
    rng = np.random.default_rng(106)
    first = np.array([0, 0, T * C - 1, 0, T * (C - 1), 7, T * C - 3, 0, 4])
    lens = np.array([T * C, 1, 1, T, T, 11, 3, 2 * T + 1, 2])
    case = iu.PackCase(rng, T=T, C=C, n=9, lens=lens, first=first)
    assert (case.span[0] == (0, T * C - 1)).all()                              # one span is the whole history of its stream
    assert (case.span[:, 0] == 0).sum() >= 3 and (case.span[:, 1] == T * C - 1).sum() >= 3
    assert (case.span[1] == (0, 0)).all() and (case.span[2] == (T * C - 1, T * C - 1)).all()
    check_pack(gpu, case)


# ------------------------------------------------------------------------------------------
# k_demo_batch
# ------------------------------------------------------------------------------------------
BATCH_ARGS = ("count", "frames", "order", "dst_start", "offset", "src_image", "src_dir", "src_action", "image", "action", "done", "mask", "episode",
              "dir8", "action8")
BATCH_OUTPUTS = {True: ("image", "action", "done", "mask", "episode"), False: ("image", "dir8", "action8")}
OUTPUT_TYPES = {"image": (np.uint8, ROW), "action": (np.int64, 1), "done": (np.uint8, 1), "mask": (np.float32, 1), "episode": (np.int64, 1),
                "dir8": (np.uint8, 1), "action8": (np.uint8, 1)}
EDGE_LENS = (1, 3, 2, 5, 4, 17, 260, 1, 6, 3)


@functools.lru_cache(maxsize=None)
def synth_store(name):
    if name == "ones":
        return iu.SynthStore(np.random.default_rng(201), np.ones(400, np.int64))
    if name == "mixed":
        rng = np.random.default_rng(202)
        lens = rng.choice([1, 2, 5, 17, 60], size=200)
        lens[rng.choice(200, size=2, replace=False)] = (250, 300)
        return iu.SynthStore(rng, lens)
    assert name == "edge"
    return iu.SynthStore(np.random.default_rng(203), np.array(EDGE_LENS))


def _order(name, store):
    D = len(store)
    if name == "one_frame":
        return np.random.default_rng(211).integers(0, D, size=300)
    if name == "mixed":
        rng = np.random.default_rng(212)
        subset = rng.permutation(D)[:120]              # a subset in shuffled order, both long demos, and 30 repeats
        return rng.permutation(np.concatenate([subset, np.flatnonzero(store.lens >= 250), rng.choice(subset, size=30)]))
    if name.endswith("identity"):
        return np.arange(D)
    if name.endswith("reversed"):
        return np.arange(D)[::-1]
    if name.endswith("last5"):
        return np.full(5, D - 1)
    return {"single_len1": [0], "single_len3": [1], "single_longest": [6], "tail_mod1": [1, 2], "tail_mod2": [3, 0], "tail_mod3": [2, 3],
            "tail_long_mod3": [6, 1]}[name]


BATCH_CASES = {"one_frame": "ones", "mixed": "mixed", "single_len1": "edge", "single_len3": "edge", "single_longest": "edge", "tail_mod1": "edge",
               "tail_mod2": "edge", "tail_mod3": "edge", "tail_long_mod3": "edge", "mixed_identity": "mixed", "mixed_reversed": "mixed",
               "mixed_last5": "mixed", "edge_identity": "edge", "edge_reversed": "edge", "edge_last5": "edge"}


@functools.lru_cache(maxsize=None)
def batch_case(name):
    """Built once, reference included, and shared by the pin test and both forms of the device test."""
    store = synth_store(BATCH_CASES[name])
    return iu.BatchCase(store, _order(name, store))


def batch_preconditions(name, case):
    """What the case is there for, computed from its inputs."""
    store, order, lens = case.store, case.order, case.store.lens[case.order]
    assert case.frames == lens.sum() and case.frames <= 6000
    if name == "one_frame":
        assert len(store) == 400 and (store.lens == 1).all() and len(order) == 300 and len(set(order)) < 300
        assert max(iu.runs_per_block(case.dst_start)) >= 56, iu.runs_per_block(case.dst_start)
    if BATCH_CASES[name] == "mixed":
        long_ones = store.lens >= 250
        assert len(store) == 200 and long_ones.sum() == 2 and set(store.lens[~long_ones]) == {1, 2, 5, 17, 60}
    if name == "mixed":
        assert len(set(order)) < len(order) <= len(store) and sorted(order) != list(order)
        src = {int(store.offset[k]) * ROW % 16 for k in order}
        dst = {int(s) * ROW % 16 for s in case.dst_start[:-1]}
        assert len(src) == 16 and len(dst) == 16, (sorted(src), sorted(dst))   # demos begin at every byte phase on both sides
        assert set(lens) >= {1, 2, 5, 17, 60} and lens.max() >= 250
    if name.startswith("single"):
        assert len(order) == 1 and case.frames == {"single_len1": 1, "single_len3": 3, "single_longest": store.lens.max()}[name]
        assert name != "single_longest" or iu.blocks_inside_one_run(case.dst_start) >= 1
    if name.startswith("tail"):
        assert case.frames % 4 == {"tail_mod1": 1, "tail_mod2": 2, "tail_mod3": 3, "tail_long_mod3": 3}[name] and case.frames * ROW % 16 != 0
        assert (case.frames * ROW > iu.BLOCK_BYTES) == (name == "tail_long_mod3")
    if name.endswith("identity"):
        assert list(order) == list(range(len(store))) and np.array_equal(case.dst_start, store.offset)
    if name.endswith("reversed"):
        assert list(order) == list(range(len(store)))[::-1]
    if name.endswith("last5"):
        assert list(order) == [len(store) - 1] * 5 and store.offset[order[0]] + lens[0] == store.frames      # the source run ends at the store's last byte


@pytest.mark.parametrize("name", sorted(BATCH_CASES))
def test_batch_reference_equals_the_host_gather(name):
    """The numpy reference of k_demo_batch = the host path of `imitation._gather` on the same synthetic cases, in both forms."""
    from babyai_amd.imitation import _gather
    case = batch_case(name)
    batch_preconditions(name, case)
    store, want = case.store, case.expect
    src = [torch.as_tensor(a) for a in (store.offset, case.order, case.dst_start)]
    data = [torch.as_tensor(store.image).reshape(-1, 7, 7, 3), torch.as_tensor(store.direction), torch.as_tensor(store.action)]
    image, action, done, mask, episode = _gather(*src, case.frames, *data, True)
    assert image.dtype == torch.uint8 and np.array_equal(image.numpy().reshape(-1, ROW), want["image"])
    assert action.dtype == torch.int64 and np.array_equal(action.numpy(), want["action"])
    assert done.dtype == torch.bool and np.array_equal(done.numpy(), want["done"].astype(bool))
    assert mask.dtype == torch.float32 and mask.shape == (case.frames, 1) and np.array_equal(mask.numpy()[:, 0], want["mask"])
    assert episode.dtype == torch.int64 and np.array_equal(episode.numpy(), want["episode"])
    image, direction, action = _gather(*src, case.frames, *data, False)
    assert np.array_equal(image.numpy().reshape(-1, ROW), want["image"])
    assert direction.dtype == torch.uint8 and np.array_equal(direction.numpy(), want["dir8"])
    assert action.dtype == torch.uint8 and np.array_equal(action.numpy(), want["action8"])


def batch_setup(device, case, batch_form):
    """As pack_setup, for bbai_demo_batch in one of its two forms (the other form's outputs are NULL)."""
    store = case.store
    keep = {"order": upload(case.order, device), "dst_start": upload(case.dst_start, device), "offset": upload(store.offset, device),
            "src_image": upload(store.image, device), "src_dir": upload(store.direction, device), "src_action": upload(store.action, device)}
    outs = {k: Guarded(case.frames * OUTPUT_TYPES[k][1] * np.dtype(OUTPUT_TYPES[k][0]).itemsize, device) for k in BATCH_OUTPUTS[batch_form]}
    args = {k: None for k in BATCH_ARGS}
    args.update({"count": len(case.order), "frames": case.frames})
    args.update({k: t.data_ptr() for k, t in keep.items()})
    args.update({k: o.ptr for k, o in outs.items()})
    return args, outs, keep


def call_batch(device, args):
    from babyai_amd.engine import load_library
    lib = load_library()
    with torch.cuda.device(device):
        return lib, lib.bbai_demo_batch(*[args[k] for k in BATCH_ARGS], current_stream(device))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["batch_form", "store_form"])
@pytest.mark.parametrize("name", sorted(BATCH_CASES))
def test_batch_kernel_equals_the_reference(gpu, name, form):
    from babyai_amd.engine import _check
    case = batch_case(name)
    batch_preconditions(name, case)
    batch_form = form == "batch_form"
    args, outs, keep = batch_setup(gpu, case, batch_form)
    lib, rc = call_batch(gpu, args)
    _check(lib, rc, "bbai_demo_batch")
    torch.cuda.current_stream(gpu).synchronize()
    for k in BATCH_OUTPUTS[batch_form]:
        dtype, width = OUTPUT_TYPES[k]
        got = outs[k].result(dtype, case.frames, width)
        want = case.expect[k].reshape(case.frames, width)
        assert got.dtype == want.dtype and np.array_equal(got, want), (k, np.flatnonzero((got != want).any(axis=1))[:8])
    del keep


# ------------------------------------------------------------------------------------------
# Argument checks: BBAI_ERR_ARG with a message, nothing launched, the outputs as they were.  Only valid device pointers, pointers
# into the guarded buffers, or NULL are passed.
# ------------------------------------------------------------------------------------------
def refused(lib, entry, rc, outs, device):
    """`entry` of `lib` just returned rc for a call that must be refused.  The message must be this call's (it begins with the entry's
    name): the caller left another entry's message behind first."""
    message = lib.bbai_last_error().decode()
    torch.cuda.synchronize(device)
    assert rc == BBAI_ERR_ARG, rc
    assert message.startswith(entry + ": ") and len(message) > len(entry) + 2 and message != STALE, message
    assert all(o.untouched() for o in outs.values())


STALE = "bbai_gae: null pointer or empty rollout"


def leave_another_message(lib):
    """bbai_last_error keeps the latest message: make the latest one bbai_gae's, so that a refusal without a message of its own shows."""
    assert lib.bbai_gae(0, 0, None, None, None, None, None, 0.99, 0.95, None, None, None) == BBAI_ERR_ARG
    assert lib.bbai_last_error().decode() == STALE


PACK_BAD = [("image", "+8"), ("direction", "+8"), ("action", "+8"), ("tokens", "+8"), ("frames", 6), ("chunk_steps", 0), ("chunks", None),
            ("span", None), ("offset", None), ("image", None), ("tokens", None), ("n", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("key,value", PACK_BAD, ids=["%s_%s" % (k, v) for k, v in PACK_BAD])
def test_pack_refuses_bad_arguments(gpu, key, value):
    from babyai_amd.engine import load_library
    case = iu.PackCase(np.random.default_rng(301), T=4, C=3, n=7, lens=np.array((3, 1, 1, 1, 2, 1, 1)))
    args, outs, keep = pack_setup(gpu, case)
    if key == "frames":
        assert value < case.n
    args[key] = args[key] + 8 if value == "+8" else value
    leave_another_message(load_library())
    lib, rc = call_pack(gpu, args)
    refused(lib, "bbai_demo_pack", rc, outs, gpu)
    del keep


# (form, argument, value); "other" = a valid, guarded buffer where the form wants NULL
BATCH_BAD = [(True, "image", "+8"), (True, "action", "+8"), (True, "done", "+8"), (True, "mask", "+8"), (True, "episode", "+8"),
             (False, "image", "+8"), (False, "dir8", "+8"), (False, "action8", "+8"), (True, "frames", 1), (False, "frames", 1),
             (True, "dir8", "other"), (True, "action8", "other"), (False, "action", "other"), (False, "episode", "other"),
             (True, "all", None), (False, "all", None), (True, "done", None), (False, "dir8", None), (False, "src_dir", None),
             (True, "order", None), (True, "dst_start", None), (True, "offset", None), (False, "order", None), (True, "src_image", None),
             (True, "image", None), (True, "count", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("batch_form,key,value", BATCH_BAD, ids=["%s_%s_%s" % ("batch" if f else "store", k, v) for f, k, v in BATCH_BAD])
def test_batch_refuses_bad_arguments(gpu, batch_form, key, value):
    from babyai_amd.engine import load_library
    case = batch_case("tail_mod3")
    assert len(case.order) == 2 and case.frames == 7
    args, outs, keep = batch_setup(gpu, case, batch_form)
    if value == "other":                        # both forms' outputs at once
        outs[key] = Guarded(case.frames * 8, gpu)
        args[key] = outs[key].ptr
    elif key == "all":                          # neither form's outputs
        for k in BATCH_OUTPUTS[batch_form][1:]:
            args[k] = None
    else:
        if key == "frames":
            assert value < len(case.order)
        args[key] = args[key] + 8 if value == "+8" else value
    leave_another_message(load_library())
    lib, rc = call_batch(gpu, args)
    refused(lib, "bbai_demo_batch", rc, outs, gpu)
    del keep


@pytest.mark.gpu
def test_batch_form_needs_no_src_dir(gpu):
    """The one NULL among the inputs that is no error: the batch form never reads the directions."""
    from babyai_amd.engine import _check
    case = batch_case("tail_mod3")
    args, outs, keep = batch_setup(gpu, case, True)
    args["src_dir"] = None
    lib, rc = call_batch(gpu, args)
    _check(lib, rc, "bbai_demo_batch")
    torch.cuda.current_stream(gpu).synchronize()
    for k in BATCH_OUTPUTS[True]:
        dtype, width = OUTPUT_TYPES[k]
        assert np.array_equal(outs[k].result(dtype, case.frames, width), case.expect[k].reshape(case.frames, width)), k
    del keep
