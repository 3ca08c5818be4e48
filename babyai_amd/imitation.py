"""Demonstrations that stay on the device: the imitation loop's twin of `rollout.DeviceRollout`.

The reference trains on demonstrations in `babyai/imitation.py`: a list of `(mission, packed images, directions, actions)`
tuples (scripts/make_agent_demos.py:111-112) that every batch unpacks into Python lists of `(obs dict, action, done)`
(`utils/demos.py:38-64 transform_demos`), sorts, flattens into a numpy object array and re-tokenises with a regex on every
model call (`format.py:59-119`).  Here the same data never becomes Python objects:

    store = DemoStore.collect("BabyAI-GoToLocal-v0", 100000, seed=0)          # the device expert; or DemoStore.from_reference(demos)
    train, valid = store.select(perm[:90000]), store.select(perm[90000:])
    log = run_epoch(acmodel, train, torch.randperm(len(train)), batch_size=256, recurrence=20, entropy_coef=0.01, optimizer=opt)

`DemoStore` keeps D demonstrations with F frames as flat tensors (image uint8[F,7,7,3], direction / action uint8[F], tokens
uint8[D,72] in `missions.VOCAB` ids, offset int64[D+1] on the device and mirrored on the host); `store.batch(indices)` builds
the flat batch of imitation.py:226-251 and `run_batch` / `run_epoch` are `run_epoch_recurrence_one_batch` / `run_epoch_recurrence`
over it (pinned to the reference's own functions by tests/test_imitation_host.py).  ROCm tensors go through the kernels of
babyai_amd/csrc/bbai_demo.hpp (include/bbai.h bbai_demo_spans / bbai_demo_pack / bbai_demo_batch); host tensors take the same
steps in torch ops, as `rollout.gae_env_major` does, so that the pin tests run without a GPU.

`DemoStore.collect_seeds` (one demonstration per LISTED seed, a pool of envs playing the list), `DemoStore.extend` and
`grow_training_set` are scripts/train_intelligent_expert.py:106-176 on the same footing (bbai_demo_jobs / bbai_demo_pack_list).

`DemoStore.replay` plays a store back, every demo in the episode its seed starts, and reports per demo whether the engine reproduces it
frame for frame and what it returns: `DemoAgent` (babyai/utils/agent.py:101-137) and scripts/evaluate.py:45-57 for a whole store on a pool
of envs (include/bbai_demo_replay.h bbai_demo_replay_feed / bbai_demo_replay_judge).
"""
import ctypes

import numpy as np

from . import missions
from .preprocess import TensorDict, remap_table

TOK_MAX = 72


def _launch(entry, *args):
    """One call of a handle-free entry of include/bbai.h on the current stream of its tensors' device.  A tensor argument goes in as its
    pointer, `(tensor, dtype)` as its pointer after a check of the type, None as a null pointer, anything else as it is; the stream goes
    last.  Every tensor must be contiguous and on the first one's device."""
    import torch
    from .engine import load_library, _check
    args = [a if isinstance(a, tuple) else (a, None) for a in args]
    dev = next(a.device for a, _ in args if isinstance(a, torch.Tensor))
    for a, dt in args:
        assert not isinstance(a, torch.Tensor) or (a.is_contiguous() and a.device == dev and dt in (None, a.dtype)), entry
    with torch.cuda.device(dev):
        lib = load_library()
        _check(lib, getattr(lib, entry)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a, _ in args],
                                        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), entry)


def _store_buffers(frames, demos, dev):
    """Fresh image, direction, action and token buffers of a store of `demos` demonstrations with `frames` frames."""
    import torch
    u8 = dict(dtype=torch.uint8, device=dev)
    return torch.empty((frames, 7, 7, 3), **u8), torch.empty(frames, **u8), torch.empty(frames, **u8), torch.empty((demos, TOK_MAX), **u8)


def demo_spans(done, gave_up, reward, g0, filter_steps, last_done, open_, span, open_count=None):
    """`demos.scan_chunk` on tensors: one chunk of rollout history ([chunk, n] uint8 / uint8 / float32) and the carry
    (last_done int32[n], open_ uint8[n], span int32[n, 2]), updated in place.  ROCm tensors: k_demo_spans, and the number of
    streams still open is left in `open_count` (int64[1] on the device) and returned as that tensor -- reading it is the one
    synchronisation of a chunk.  Host tensors: the same scan in torch ops, returns a 0-d tensor."""
    import torch
    chunk, n = done.shape
    if done.is_cuda:
        if open_count is None:
            open_count = torch.zeros(1, dtype=torch.int64, device=done.device)
        _launch("bbai_demo_spans", n, chunk, (done, torch.uint8), (gave_up, torch.uint8), (reward, torch.float32), int(g0), int(filter_steps),
                (last_done, torch.int32), (open_, torch.uint8), (span, torch.int32), open_count)
        return open_count
    done_b = done != 0
    idx = torch.arange(g0, g0 + chunk, dtype=torch.int32).unsqueeze(1)                       # [chunk, 1]
    ends = torch.cummax(torch.where(done_b, idx, torch.full_like(idx, -1)), dim=0).values   # latest episode end at or before each step
    ends = torch.maximum(ends, last_done.unsqueeze(0))
    before = torch.cat([last_done.unsqueeze(0), ends[:-1]], dim=0)                           # ... before each step
    ok = done_b & (gave_up == 0) & (reward > 0)
    if filter_steps:
        ok &= (idx - before) <= filter_steps
    found = ok.any(dim=0) & (open_ != 0)
    first = ok.to(torch.uint8).argmax(dim=0)
    cols = found.nonzero().reshape(-1)
    span[cols, 0] = before[first[cols], cols] + 1
    span[cols, 1] = (g0 + first[cols]).to(torch.int32)
    open_[cols] = 0
    last_done.copy_(ends[-1])
    return (open_ != 0).sum()


def _gather(offset, order, dst_start, frames, src_image, src_dir, src_action, batch_form):
    """The segmented copy behind `batch` and `select`: demos `order` (int64[B] on the store's device) of a store laid end to
    end.  Returns (image, action int64, done, mask, episode_ids) or (image, direction, action uint8)."""
    import torch
    dev = src_image.device
    B = int(order.shape[0])
    image = torch.empty((frames, 7, 7, 3), dtype=torch.uint8, device=dev)
    if batch_form:
        out = [torch.empty(frames, dtype=torch.int64, device=dev), torch.empty(frames, dtype=torch.bool, device=dev),
               torch.empty((frames, 1), dtype=torch.float32, device=dev), torch.empty(frames, dtype=torch.int64, device=dev)]
    else:
        out = [torch.empty(frames, dtype=torch.uint8, device=dev), torch.empty(frames, dtype=torch.uint8, device=dev)]
    if src_image.is_cuda:
        _launch("bbai_demo_batch", B, frames, order, dst_start, offset, src_image, src_dir, src_action, image,
                *(out + [None, None] if batch_form else [None] * 4 + out))
        return [image] + out
    lens = dst_start[1:] - dst_start[:-1]
    episode = torch.repeat_interleave(torch.arange(B), lens)
    within = torch.arange(frames) - dst_start[:-1][episode]
    src = offset[order][episode] + within
    image.copy_(src_image[src])
    if batch_form:
        out[0].copy_(src_action[src])
        out[1].copy_(within == lens[episode] - 1)
        out[2].copy_((within != 0).to(torch.float32).unsqueeze(1))
        out[3].copy_(episode)
    else:
        out[0].copy_(src_dir[src])
        out[1].copy_(src_action[src])
    return [image] + out


class DemoBatch(object):
    """The flat batch of imitation.py:226-251: demos longest first (stable), frames of demo b at `inds[b] : inds[b] + lengths[b]`.
    image uint8[Fb,7,7,3], action int64[Fb], done bool[Fb], mask float32[Fb,1], episode_ids int64[Fb], inds int64[B],
    instr int64[B,L'] on the device; order (the store's demo numbers in batch order), lengths and counts on the host."""

    def __init__(self, image, action, done, mask, episode_ids, inds, instr, order, lengths):
        self.image, self.action, self.done, self.mask, self.episode_ids = image, action, done, mask, episode_ids
        self.inds, self.instr, self.order, self.lengths = inds, instr, order, lengths
        self.num_frames = int(lengths.sum())
        # counts[t] = demos with more than t frames = how many of the sorted demos the reference's first loop still visits at step t
        self.counts = np.searchsorted(-lengths, -np.arange(int(lengths[0])), side="left") if len(lengths) else np.zeros(0, np.int64)

    def __len__(self):
        return len(self.lengths)

    def active(self, t):
        """Flat indices of step t of every demo that has one (imitation.py:257-278): longest first, so a prefix of `inds`."""
        return self.inds[:int(self.counts[t])] + t

    def starting_indexes(self, recurrence):
        """imitation.py:183-187"""
        import torch
        idx = torch.arange(0, self.num_frames, recurrence, device=self.image.device)
        return idx if self.num_frames % recurrence == 0 else idx[:-1]


class DemoStore(object):
    def __init__(self, image, direction, action, tokens, offset_host=None, offset=None):
        """`offset_host` (int64[D + 1] on the host) or `offset` (the same on the store's device: the host mirror is then read when it is
        first asked for) or both."""
        import torch
        self.image, self.direction, self.action, self.tokens = image, direction, action, tokens
        self.device = image.device
        self._count, self._frames = int(tokens.shape[0]), int(image.shape[0])
        assert image.shape[0] == direction.shape[0] == action.shape[0]
        if offset_host is not None:
            self._offset_host = np.ascontiguousarray(offset_host, dtype=np.int64)
            assert self._frames == int(self._offset_host[-1]) and self._count == len(self._offset_host) - 1
            offset = torch.as_tensor(self._offset_host, device=image.device) if offset is None else offset
        else:
            self._offset_host = None
        assert offset.shape[0] == self._count + 1 and offset.dtype == torch.int64 and offset.device == image.device
        self.offset = offset
        self._ntok = None
        self._buf = None                        # extend(): the buffers with room to grow; the attributes above are views of their filled prefix

    def __len__(self):
        return self._count

    @property
    def num_frames(self):
        return self._frames

    @property
    def offset_host(self):
        if self._offset_host is None:
            self._offset_host = np.ascontiguousarray(self.offset.cpu().numpy(), dtype=np.int64)
        return self._offset_host

    @property
    def lengths(self):
        return np.diff(self.offset_host)

    @property
    def capacity(self):
        """(frames, demos) the store can hold before `extend` allocates again"""
        return (int(self._buf["direction"].shape[0]), int(self._buf["tokens"].shape[0])) if self._buf else (self._frames, self._count)

    def _reserve(self, frames, demos):
        """Buffers for at least `frames` / `demos`; a buffer that is too small is replaced by one of TWICE what is needed, so that a run of
        extends copies every frame a bounded number of times.  The image buffer keeps 16 spare bytes behind its last frame: k_demo_batch
        reads the aligned 16-byte words around its runs."""
        import torch
        cap_f, cap_d = self.capacity if self._buf else (-1, -1)
        if frames <= cap_f and demos <= cap_d:
            return
        new_f = cap_f if frames <= cap_f else 2 * frames
        new_d = cap_d if demos <= cap_d else 2 * demos
        new_f, new_d = max(new_f, 1), max(new_d, 1)
        u8 = dict(dtype=torch.uint8, device=self.device)
        buf = {"image": torch.empty(new_f * 147 + 16, **u8), "direction": torch.empty(new_f, **u8), "action": torch.empty(new_f, **u8),
               "tokens": torch.empty((new_d, TOK_MAX), **u8), "offset": torch.zeros(new_d + 1, dtype=torch.int64, device=self.device)}
        F, D = self._frames, self._count
        buf["image"][:F * 147].copy_(self.image.reshape(-1))
        buf["direction"][:F].copy_(self.direction)
        buf["action"][:F].copy_(self.action)
        buf["tokens"][:D].copy_(self.tokens)
        buf["offset"][:D + 1].copy_(self.offset)
        self._buf = buf
        self._view()

    def _view(self):
        b, F, D = self._buf, self._frames, self._count
        self.image, self.direction, self.action = b["image"][:F * 147].view(F, 7, 7, 3), b["direction"][:F], b["action"][:F]
        self.tokens, self.offset = b["tokens"][:D], b["offset"][:D + 1]

    def extend(self, other):
        """Append the demonstrations of `other` (a store on the same device), in place: `train_demos.extend(new_demos)` of
        scripts/train_intelligent_expert.py:171.  Nothing crosses to the host; the host mirror of `offset` follows if both stores have one."""
        if len(other) == 0:
            return self
        assert other.device == self.device, "extend: both stores on one device"
        F, D, f, d = self._frames, self._count, other.num_frames, len(other)
        self._reserve(F + f, D + d)
        b = self._buf
        b["image"][F * 147:(F + f) * 147].copy_(other.image.reshape(-1))
        b["direction"][F:F + f].copy_(other.direction)
        b["action"][F:F + f].copy_(other.action)
        b["tokens"][D:D + d].copy_(other.tokens)
        b["offset"][D + 1:D + d + 1].copy_(other.offset[1:] + F)
        if self._offset_host is not None and other._offset_host is not None:
            self._offset_host = np.concatenate([self._offset_host, other._offset_host[1:] + F])
        else:
            self._offset_host = None
        self._frames, self._count, self._ntok = F + f, D + d, None
        self._view()
        return self

    @classmethod
    def empty(cls, device="cpu"):
        import torch
        z = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device=device)
        return cls(z(0, 7, 7, 3), z(0), z(0), z(0, TOK_MAX), np.zeros(1, np.int64))

    # ---- ways in ----
    @classmethod
    def _from_arrays(cls, image, direction, action, tokens, offset, device="cpu"):
        import torch
        t = [torch.as_tensor(np.ascontiguousarray(a, dtype=np.uint8), device=device) for a in (image, direction, action, tokens)]
        return cls(t[0].reshape(-1, 7, 7, 3), t[1].reshape(-1), t[2].reshape(-1), t[3].reshape(-1, TOK_MAX), offset)

    @classmethod
    def from_reference(cls, demos, device="cpu", unpack=None):
        """From the reference's list of (mission, images, directions, actions); `unpack=blosc.unpack_array` for packed images."""
        images = [np.asarray(unpack(d[1]) if unpack else d[1], dtype=np.uint8).reshape(-1, 7, 7, 3) for d in demos]
        lens = [len(d[3]) for d in demos]
        for im, d, n in zip(images, demos, lens):
            assert im.shape[0] == len(d[2]) == n, "error transforming demos"       # utils/demos.py:55
        tokens = np.zeros((len(demos), TOK_MAX), dtype=np.uint8)
        for k, d in enumerate(demos):
            ids = missions.tokenize(d[0])
            tokens[k, :len(ids)] = ids
        cat = np.concatenate
        return cls._from_arrays(cat(images) if images else np.zeros((0, 7, 7, 3), np.uint8), cat([np.asarray(d[2], np.uint8) for d in demos]),
                               cat([np.asarray(d[3], np.uint8) for d in demos]), tokens, np.concatenate([[0], np.cumsum(lens)]), device)

    @classmethod
    def load(cls, path, device="cpu"):
        with np.load(path) as f:
            return cls._from_arrays(f["image"], f["direction"], f["action"], f["tokens"], f["offset"], device)

    @classmethod
    def collect(cls, env_name, n_episodes, seed, device="cuda:0", batch=32768, filter_steps=0, max_steps=None):
        """The contract of `demos.generate_demos` (demo k = the first episode of stream seed + k that the expert solves), with the
        result left on the device: per chunk of rollout history one counter crosses PCIe, per batch of streams its lengths."""
        import torch
        parts = [_collect_batch(env_name, seed + start, min(batch, n_episodes - start), device, filter_steps, max_steps)
                 for start in range(0, n_episodes, batch)]
        if len(parts) == 1:
            return cls(*parts[0])
        lens = np.concatenate([np.diff(p[4]) for p in parts])
        return cls(*[torch.cat([p[i] for p in parts]) for i in range(4)], np.concatenate([[0], np.cumsum(lens)]))

    @classmethod
    def collect_seeds(cls, env_name, seeds, device="cuda:0", pool=32768, chunk=None, env=None, reseed_levels=None):
        """One demonstration per LISTED seed (`generate_demos(env_name, seeds)` of scripts/train_intelligent_expert.py:106-147): for every
        seeds[j], in order, the episode that `env.seed(seeds[j]); env.reset()` starts, played by the expert, kept iff it ends with
        reward > 0 and the expert did not give up.  -> (store of the kept demonstrations in the order of `seeds`, kept = their positions in
        `seeds`, int64 on the host).  min(pool, len(seeds)) envs play the list (see _collect_seeds).  `reseed_levels` (None = the engine's
        option as it stands: whole look-ahead rings): the `levels=` of the pool's reseeds; with 1 a pool env plays its seed's one episode and
        parks until the round's reseed instead of playing on through rows nobody reads -- the same (store, kept), less generator and
        expert work."""
        return _collect_seeds(cls, env_name, seeds, device, pool, chunk, env, reseed_levels)

    def replay(self, env_name, seeds, device="cuda:0", pool=32768, reseed_every=None, poll_every=16, env=None):
        """Play every demonstration back in the episode its seed starts and report, per demo, whether the engine reproduces it: `DemoAgent`
        (babyai/utils/agent.py:101-137) and the `--demos` evaluation built on it (scripts/evaluate.py:45-57), for the whole store at once and
        without the assert -- a mismatch is counted, the recorded actions go on being applied, frames behind `done` are never compared.
        `seeds`: one per demo (what `engine.seeds_u64` takes; ValueError for another number): demo j is replayed in the episode that
        `env.seed(seeds[j]); env.reset()` starts -- after `store, kept = DemoStore.collect_seeds(name, s)` that is `np.asarray(s)[kept]`.
        -> DemoReplay (played, done_at, return64, mismatches, first_mismatch, mission_ok per demo; `.exact`, `.logs()`).
        min(pool, D') envs (auto_reset=False) play the D' non-empty demos -- a zero-length demo is reported as played = done_at = 0 --; an env
        that has finished one waits for the next reseed tick.  `reseed_every` = r: the free envs claim their next demos and are reseeded
        (levels=1) every r ticks; None = 16, chosen from profiles/demo_replay/demo_replay_bench.jsonl (tools/demo_replay_bench.py): a reseed
        call costs 0.4-0.7 ms of device time whatever it finds to do, ten times a tick's feed + step + judge, so at pools 4 096 / 32 768
        r = 16 replays BossLevel (84 frames per demo) 1.74x / 1.23x as fast as r = 4 and 4.8x / 2.1x as fast as r = 1, and GoToLocal (5
        frames per demo, where waiting costs most) within 5 % / 2 % of its best, r = 4; at pool 131 072 r makes no difference.
        `poll_every`: the host reads the two counters every that many ticks and stops when every demo has finished; nothing else
        synchronises.  The results do not depend on pool, reseed_every or poll_every.  RuntimeError when (ceil(D' / P) + 1) * (the longest
        demo + r) + poll_every ticks do not finish the store.  `env`: a prepared pool as for collect_seeds(env=...) -- num_envs (<= D'),
        device, image, direction, reward64, done, instr, step(actions) that honours HOLD bytes, reseed(ids, seeds, levels=), close() --
        created on the seeds of the first num_envs non-empty demos, auto_reset=False, token rows on, reset() behind it; it stays the
        caller's.  A pool in the reference's done-action mode is refused (ValueError): a store does not say whether a recorded `done` was
        the enum member."""
        return _replay(self, env_name, seeds, device, pool, reseed_every, poll_every, env)

    # ---- ways out ----
    def to_reference(self, pack=None):
        """The reference's tuples; with `DemoStore.collect` in front of it, interchangeable with `demos.generate_demos`."""
        img, dirs, acts = self.image.cpu().numpy(), self.direction.cpu().numpy().tolist(), self.action.cpu().numpy().tolist()
        toks, ends = self.tokens.cpu().numpy(), self.offset_host.tolist()
        text, out = {}, []
        for k in range(len(self)):
            key = toks[k].tobytes()
            mission = text.get(key)
            if mission is None:
                mission = text[key] = missions.detokenize(key)
            lo, hi = ends[k], ends[k + 1]
            stack = img[lo:hi]
            out.append((mission, pack(stack) if pack else stack, dirs[lo:hi], acts[lo:hi]))
        return out

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, image=self.image.cpu().numpy(), direction=self.direction.cpu().numpy(), action=self.action.cpu().numpy(),
                     tokens=self.tokens.cpu().numpy(), offset=self.offset_host)

    def _indices(self, indices):
        """(host int64 array, device int64 tensor) of demo numbers from a host sequence or a tensor"""
        import torch
        if isinstance(indices, torch.Tensor):
            dev = indices.to(device=self.device, dtype=torch.int64).contiguous()
            host = indices.cpu().numpy().astype(np.int64)        # (a device tensor is read back here, B numbers: the sort by length and the
                                                                 #  frame count of the result are the host's; pass host indices to avoid the wait)
        else:
            host = np.ascontiguousarray(indices, dtype=np.int64)
            dev = torch.as_tensor(host, device=self.device)
        if host.size and (host.min() < 0 or host.max() >= len(self)):
            raise IndexError("demo index out of range")
        return host, dev

    def select(self, indices):
        """A new store holding demos `indices` in that order (device copy): the train / validation split."""
        import torch
        host, order = self._indices(indices)
        start = np.concatenate([[0], np.cumsum(self.lengths[host])]).astype(np.int64)
        if host.size == 0:
            return DemoStore(self.image[:0], self.direction[:0], self.action[:0], self.tokens[:0], start)
        image, direction, action = _gather(self.offset, order, torch.as_tensor(start, device=self.device), int(start[-1]),
                                           self.image, self.direction, self.action, False)
        return DemoStore(image, direction, action, self.tokens[order], start)

    def _token_counts(self):
        """Tokens per mission, on the host (one read of D numbers, cached)."""
        if self._ntok is None:
            self._ntok = (self.tokens != 0).sum(dim=1).cpu().numpy()
        return self._ntok

    def batch(self, indices, vocab=None):
        """The flat batch of demos `indices` (imitation.py:226-251).  `vocab`: None = the engine's fixed ids; a reference vocabulary
        ({word: id} or the path of a vocab.json) = ids remapped as `TensorObssPreprocessor(env, vocab=...)` does."""
        import torch
        host, _ = self._indices(indices)
        if host.size == 0:
            raise ValueError("empty batch")
        lens = self.lengths[host]
        rank = np.argsort(-lens, kind="stable")                  # batch.sort(key=len, reverse=True) keeps the given order among equals
        order_h, lens = host[rank], lens[rank]
        start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        order = torch.as_tensor(order_h, device=self.device)
        start_d = torch.as_tensor(start, device=self.device)
        image, action, done, mask, episode = _gather(self.offset, order, start_d, int(start[-1]), self.image, self.direction, self.action, True)
        width = max(int(self._token_counts()[order_h].max()), 0)
        instr = self.tokens[order][:, :width].to(torch.int64)    # padded to the batch's longest mission (format.py:59-75)
        if vocab is not None:
            if not isinstance(vocab, dict):
                import json
                with open(vocab) as f:
                    vocab = json.load(f)
            instr = torch.as_tensor(remap_table(vocab)[0], dtype=torch.int64, device=self.device)[instr]
        return DemoBatch(image, action, done, mask, episode, start_d[:-1], instr, order_h, lens)


def _collect_batch(env_name, seed, n, device, filter_steps, max_steps):
    """One batch of streams of `DemoStore.collect` (demos._generate_batch with the scan and the gather left on the device)."""
    import torch
    from .engine import BatchedBabyAIEnv
    env = BatchedBabyAIEnv(env_name, n, device=device, seeds=[seed + k for k in range(n)], auto_reset=True)
    try:
        env.enable_instr_tokens()
        env.reset()
        dev = env.device
        budget = max_steps if max_steps is not None else 64 * env.max_steps_bound
        chunk = collect_chunk(env.max_steps_bound, budget)
        free_b, _ = torch.cuda.mem_get_info(dev)
        chunk_bytes = chunk * n * (147 + 72 + 6 + 4)
        max_chunks = max(2, int(free_b // 2 // max(1, chunk_bytes)))          # the history's memory bound of generate_demos
        with torch.cuda.device(dev):
            last_done = torch.full((n,), -1, dtype=torch.int32, device=dev)
            open_ = torch.ones(n, dtype=torch.uint8, device=dev)
            span = torch.full((n, 2), -1, dtype=torch.int32, device=dev)
            counter = torch.zeros(1, dtype=torch.int64, device=dev)
        hist, g0, still = [], 0, n
        while still and g0 < budget:
            if len(hist) >= max_chunks:
                raise RuntimeError("no solvable episode found for %d stream(s) within the history memory budget (%d chunks of %d steps x %d "
                                   "streams = %.1f GB on the device): use a smaller `batch`" % (still, len(hist), chunk, n, len(hist) * chunk_bytes / 1e9))
            r = env.bot_rollout(chunk, tokens=True)
            hist.append(r)
            demo_spans(r["done"], r["gave_up"], r["reward"], g0, filter_steps, last_done, open_, span, counter)
            still = int(counter.item())                                        # 8 bytes per chunk
            g0 += chunk
        if still:
            raise RuntimeError("no solvable episode found for %d stream(s) within the step budget" % still)
        return _pack(hist, span, chunk)
    finally:
        env.close()


def _pack(hist, span, chunk):
    """The spans of a batch of streams (int32[n, 2] on the device) in the history chunks `hist` (bot_rollout results of `chunk` steps each)
    -> (image, direction, action, tokens, offset_host): k_demo_pack."""
    import torch
    dev, n = span.device, int(span.shape[0])
    lens = (span[:, 1] - span[:, 0] + 1).to(torch.int64)
    offset = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens, 0, out=offset[1:])
    offset_host = offset.cpu().numpy()                                     # the batch's lengths: the one other read
    frames = int(offset_host[-1])
    image, direction, action, tokens = _store_buffers(frames, n, dev)
    _launch("bbai_demo_pack", n, frames, chunk, ring_table(hist), span, offset, image, direction, action, tokens)
    torch.cuda.current_stream(dev).synchronize()                       # the history may be freed (and the env closed) after this
    return image, direction, action, tokens, offset_host


def collect_chunk(max_steps_bound, budget=None):
    """Steps per bot_rollout call of `collect` and `collect_seeds`."""
    chunk = min(128, max(16, max_steps_bound // 4))
    return max(1, chunk if budget is None else min(chunk, budget))


def demo_jobs(done, gave_up, reward, g0, job, start, job_seeds, ids_out, seeds_out, records, counters):
    """One chunk of history of a pool of envs that play a list of seeds (include/bbai.h bbai_demo_jobs): done / gave_up / reward [chunk, n] of
    one bot_rollout call whose row 0 is global step g0; job int32[n] (position in the list, -1 = idle) and start int32[n] (global step the
    episode began at), updated in place; job_seeds int64[J] (the list, uint64 bit patterns); ids_out / seeds_out int64[n] = the lists for
    `reseed` (ids_out = -1 where the env claimed nothing); records int32[n, 4] = (env, first step, length, job) of the episodes kept in
    this call; counters int64[4] = job cursor (in / out), finished (running total), records and frames of this call.  ROCm tensors:
    k_demo_jobs, which hands the jobs out wave by wave in whatever order the waves arrive; host tensors: the same in torch ops, jobs in
    env order."""
    import torch
    chunk, n = done.shape
    J = int(job_seeds.shape[0])
    if done.is_cuda:
        assert job.shape[0] == start.shape[0] == ids_out.shape[0] == seeds_out.shape[0] == n and tuple(records.shape) == (n, 4) and counters.shape[0] == 4
        _launch("bbai_demo_jobs", n, chunk, (done, torch.uint8), (gave_up, torch.uint8), (reward, torch.float32), int(g0), (job, torch.int32),
                (start, torch.int32), (job_seeds, torch.int64), J, (ids_out, torch.int64), (seeds_out, torch.int64), (records, torch.int32),
                (counters, torch.int64))
        return counters
    cols = torch.arange(n)
    done_b = done != 0
    fin = done_b.any(dim=0) & (job >= 0)
    first = done_b.to(torch.uint8).argmax(dim=0)                         # the first done row of every column
    keep = fin & (gave_up[first, cols] == 0) & (reward[first, cols] > 0)
    kept = keep.nonzero().reshape(-1)
    lens = (g0 + first[kept] - start[kept] + 1).to(torch.int32)
    records[:len(kept)] = torch.stack([kept.to(torch.int32), start[kept], lens, job[kept]], dim=1)
    done_ = fin.nonzero().reshape(-1)
    nxt = int(counters[0]) + torch.arange(len(done_))
    ok = nxt < J
    ids_out.fill_(-1)
    ids_out[done_[ok]] = done_[ok]
    seeds_out[done_[ok]] = job_seeds[nxt[ok]]
    job[done_] = torch.where(ok, nxt, torch.full_like(nxt, -1)).to(torch.int32)
    start[done_[ok]] = g0 + chunk
    counters[0] += len(done_)
    counters[1] += len(done_)
    counters[2] = len(kept)
    counters[3] = int(lens.sum())
    return counters


def demo_pack_list(ring, chunk, records, frames, table=None):
    """The records of `demo_jobs` -> a store of their demonstrations, in the records' order (include/bbai.h bbai_demo_pack_list).  `ring`: the
    R history slots (bot_rollout results of `chunk` steps with tokens), global step g = row g % chunk of slot (g // chunk) % R; records
    int32[k, 4] on the slots' device; frames = the sum of their lengths (known from demo_jobs' counters: nothing is read back here).
    `table`: the device table of the slots' pointers, if the caller keeps one."""
    import torch
    dev, R, k = records.device, len(ring), int(records.shape[0])
    n = int(ring[0]["done"].shape[1])
    offset = torch.zeros(k + 1, dtype=torch.int64, device=dev)
    torch.cumsum(records[:, 2].to(torch.int64), 0, out=offset[1:])
    if records.is_cuda:
        image, direction, action, tokens = _store_buffers(frames, k, dev)
        _launch("bbai_demo_pack_list", k, frames, n, chunk, R, ring_table(ring) if table is None else table, (records, torch.int32), offset,
                image, direction, action, tokens)
        return DemoStore(image, direction, action, tokens, offset=offset)
    rec = records.to(torch.int64)
    demo = torch.repeat_interleave(torch.arange(k), rec[:, 2])
    g = rec[demo, 1] + torch.arange(frames) - offset[demo]
    slot, row, env = (g // chunk) % R, g % chunk, rec[demo, 0]
    hist = {key: torch.stack([r[key] for r in ring]) for key in ("image", "direction", "action", "tokens")}          # [R, chunk, n, ...]
    g1 = rec[:, 1]
    return DemoStore(hist["image"][slot, row, env], hist["direction"][slot, row, env], hist["action"][slot, row, env],
                     hist["tokens"][(g1 // chunk) % R, g1 % chunk, rec[:, 0]], offset.numpy().copy(), offset)


def ring_table(ring):
    """The device table of bbai_demo_chunk entries of history slots.  The pack kernels fetch the aligned 16-byte words around the rows they
    need (include/bbai.h): every array must start 16-byte aligned in an allocation padded to a multiple of 16 bytes, as torch's caching
    allocator hands them out (blocks start 512-byte aligned and are rounded up to 512 bytes)."""
    import torch
    keys = ("image", "direction", "action", "tokens")
    for r in ring:
        for k in keys:
            assert r[k].data_ptr() % 16 == 0
    return torch.as_tensor(np.array([[r[k].data_ptr() for k in keys] for r in ring], dtype=np.int64), device=ring[0]["image"].device)


ROUND_EVENTS = None         # measurement aid (tools/seed_demos_bench.py): a list collects (part, start event, end event) of every round of collect_seeds


class _Timed(object):
    """`with _Timed(dev, part):` brackets a part of a round by HIP events on the current stream while ROUND_EVENTS is a list."""

    def __init__(self, dev, part):
        self.on = ROUND_EVENTS is not None and dev.type == "cuda"
        self.dev, self.part = dev, part

    def __enter__(self):
        if self.on:
            import torch
            self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            self.ev[0].record(torch.cuda.current_stream(self.dev))

    def __exit__(self, *exc):
        if self.on:
            import torch
            self.ev[1].record(torch.cuda.current_stream(self.dev))
            ROUND_EVENTS.append((self.part, self.ev[0], self.ev[1]))


def _collect_seeds(cls, env_name, seeds, device, pool, chunk, env, reseed_levels=None):
    """A pool of P = min(pool, J) auto-resetting envs plays the J listed seeds, rounds of `chunk` expert steps each: bot_rollout into the next
    slot of a ring of history slots, one k_demo_jobs launch (which episodes ended, which are kept, who plays what next), one read of its four
    counters -- the round's only synchronisation --, a reseed of the envs that finished with the device lists the kernel wrote, and, if
    anything was kept, one k_demo_pack_list launch into a part that the staging store is extended by.  An env that finished goes on through
    its stream until the round ends (rows nobody reads); an episode therefore always starts on a round's first row and ends within
    max_steps_bound steps, so a ring of ceil(max_steps_bound / chunk) + 1 slots never overwrites a row that a live episode needs.  The
    staging order depends on which wave claimed what; the result -- the staging store's demos sorted by job -- does not.  `env`: any
    object with num_envs, device, max_steps_bound, bot_rollout(steps, tokens, out), reseed(ids, seeds) and close(), already created on the
    first num_envs seeds with auto-reset, token rows on and reset() behind it (the host build in the tests); pool = its size.
    `reseed_levels` = k (not None) is passed to every reseed as `levels=k` (an `env=` then needs reseed(ids, seeds, levels=)): a pool env plays
    k levels of its seed's stream and parks -- frozen: its steps write no `done` / `reward` rows, the expert answers `done` for it -- until the
    round's reseed.  Only an env's FIRST done row of a round is ever read, and the rows in front of it were written by the live env; an env
    without a job (idle: its column may be parked, unwritten memory from its first row on) is skipped by demo_jobs whatever its column holds.
    So every k >= 1 gives the default's (store, kept).  The first round's envs come from seed() + reset(), with full rings: a pool created
    here is put into its first levels by a reseed of every env at depth k instead of by reset(), so that they park as well."""
    import torch
    from .engine import reseed_levels_arg, seeds_u64
    reseed_levels = reseed_levels_arg(reseed_levels, "collect_seeds")
    seeds_h = seeds_u64(seeds, "collect_seeds")
    J = len(seeds_h)
    if J == 0:
        return cls.empty(env.device if env is not None else ("cpu" if not torch.cuda.is_available() else device)), np.zeros(0, np.int64)
    own = env is None
    if own:
        from .engine import BatchedBabyAIEnv
        if int(pool) < 1:
            raise ValueError("collect_seeds: pool must be at least 1")
        env = BatchedBabyAIEnv(env_name, min(int(pool), J), device=device, seeds=seeds_h[:min(int(pool), J)], auto_reset=True)
    try:
        P, dev = int(env.num_envs), torch.device(env.device)
        if P > J:
            raise ValueError("collect_seeds: %d envs for %d seeds" % (P, J))
        if own:
            env.enable_instr_tokens()
            if reseed_levels:
                env.reseed(None, seeds_h[:P], levels=reseed_levels)
            else:
                env.reset()
        bound = int(env.max_steps_bound)
        chunk = collect_chunk(bound) if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError("collect_seeds: chunk must be at least 1")
        R = -(-bound // chunk) + 1
        if dev.type == "cuda":
            free_b, _ = torch.cuda.mem_get_info(dev)
            need = R * chunk * P * 229
            if need > free_b // 2:
                fit = max(1, int(free_b // 2 // (R * chunk * 229)))
                raise ValueError("collect_seeds: the history ring of %d slots x %d steps x %d envs needs %.1f GB, more than half of the free device "
                                 "memory: use pool=%d or less" % (R, chunk, P, need / 1e9, fit))
        i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        job, start = torch.arange(P, **i32), torch.zeros(P, **i32)
        job_seeds = torch.as_tensor(seeds_h.view(np.int64), device=dev)
        ids_out, seeds_out = torch.full((P,), -1, **i64), torch.zeros(P, **i64)
        records = torch.zeros((P, 4), **i32)
        counters = torch.as_tensor(np.array([P, 0, 0, 0], dtype=np.int64), device=dev)
        ring = [{"image": torch.empty((chunk, P, 7, 7, 3), **u8), "direction": torch.empty((chunk, P), **u8), "action": torch.empty((chunk, P), **u8),
                 "reward": torch.empty((chunk, P), dtype=torch.float32, device=dev), "done": torch.empty((chunk, P), **u8),
                 "gave_up": torch.empty((chunk, P), **u8), "tokens": torch.empty((chunk, P, TOK_MAX), **u8)} for _ in range(R)]
        table = ring_table(ring) if dev.type == "cuda" else None
        staging, kept_records = cls.empty(dev), []
        g0 = rnd = finished = 0
        cursor = P
        while finished < J:
            if g0 + 2 * chunk > 0x7fffffff:
                raise RuntimeError("collect_seeds: the global step index would pass 2^31: use a larger pool, or fewer seeds per call")
            slot = ring[rnd % R]
            with _Timed(dev, "bot_rollout"):
                env.bot_rollout(chunk, tokens=True, out=slot)
            with _Timed(dev, "k_demo_jobs"):
                demo_jobs(slot["done"], slot["gave_up"], slot["reward"], g0, job, start, job_seeds, ids_out, seeds_out, records, counters)
            c = counters.cpu().numpy()                                          # 8 bytes per counter: the round's one synchronisation
            claimed, ended, nrec, frames = int(c[0]) - cursor, int(c[1]) - finished, int(c[2]), int(c[3])
            if claimed and cursor < J:
                with _Timed(dev, "reseed"):
                    if reseed_levels is None:
                        env.reseed(ids_out, seeds_out)
                    else:
                        env.reseed(ids_out, seeds_out, levels=reseed_levels)
            if nrec:
                rec = records[:nrec].clone()
                kept_records.append(rec)
                with _Timed(dev, "pack"):
                    part = demo_pack_list(ring, chunk, rec, frames, table)
                with _Timed(dev, "extend"):
                    staging.extend(part)
            cursor, finished = cursor + claimed, finished + ended
            g0 += chunk
            rnd += 1
        if not kept_records:
            return cls.empty(dev), np.zeros(0, np.int64)
        jobs = torch.cat(kept_records)[:, 3].cpu().numpy().astype(np.int64)
        order = np.argsort(jobs, kind="stable")
        result = staging.select(order)
        if dev.type == "cuda":
            torch.cuda.current_stream(dev).synchronize()                       # the ring may be freed (and the env closed) after this
        return result, jobs[order]
    finally:
        if own:
            env.close()


HOLD = 8                    # include/bbai.h BBAI_ACTION_HOLD
REPLAY_RESEED_EVERY = 16    # DemoStore.replay(reseed_every=None): see its docstring for the measurement behind it


def replay_feed(image, direction, instr, job, pos, store, mismatches, first_mismatch, mission_ok, actions_out, fed):
    """Before the step of a pool that plays `store` back (include/bbai_demo_replay.h bbai_demo_replay_feed): image uint8[n, 7, 7, 3], direction
    uint8[n] and instr uint8[n, 72] = the pool's current observations and token rows; job int32[n] = the demo env i plays (< 0: none), pos
    int32[n] = the frame it stands at.  An env with 0 <= job < len(store) and 0 <= pos < the demo's length is FED: its observation is compared
    with the demo's frame `pos` (a difference adds 1 to mismatches[job] and sets first_mismatch[job] = pos while that is -1), at pos == 0 its
    token row with the demo's (mission_ok[job] = 1 / 0), actions_out[i] = the recorded action and fed[i] = 1.  Every other env gets
    actions_out[i] = HOLD and fed[i] = 0.  mismatches / first_mismatch int32[D], mission_ok uint8[D], actions_out / fed uint8[n], all written
    in place.  ROCm tensors: k_demo_replay_feed; host tensors: the same in torch ops."""
    import torch
    n, D, F = int(job.shape[0]), len(store), store.num_frames
    if image.is_cuda:
        assert pos.shape[0] == actions_out.shape[0] == fed.shape[0] == direction.shape[0] == n and tuple(instr.shape) == (n, TOK_MAX)
        assert image.numel() == n * 147 and mismatches.shape[0] == first_mismatch.shape[0] == mission_ok.shape[0] == D
        _launch("bbai_demo_replay_feed", n, (image, torch.uint8), (direction, torch.uint8), (instr, torch.uint8), (job, torch.int32), (pos, torch.int32),
                D, F, (store.offset, torch.int64), (store.image, torch.uint8), (store.direction, torch.uint8), (store.action, torch.uint8),
                (store.tokens, torch.uint8), (mismatches, torch.int32), (first_mismatch, torch.int32), (mission_ok, torch.uint8),
                (actions_out, torch.uint8), (fed, torch.uint8))
        return
    j, p = job.to(torch.int64), pos.to(torch.int64)
    jc = j.clamp(0, max(D - 1, 0))
    lo = store.offset[jc]
    f = lo + p
    play = (j >= 0) & (j < D) & (p >= 0) & (f < store.offset[jc + 1]) & (f < F)
    env = play.nonzero().reshape(-1)
    d, f, p = jc[env], f[env], p[env]
    diff = (image[env].reshape(-1, 147) != store.image[f].reshape(-1, 147)).any(dim=1) | (direction[env] != store.direction[f])
    mismatches.index_add_(0, d, diff.to(torch.int32))
    new = diff & (first_mismatch[d] < 0)
    first_mismatch[d[new]] = p[new].to(torch.int32)
    at0 = p == 0
    mission_ok[d[at0]] = (instr[env[at0]] == store.tokens[d[at0]]).all(dim=1).to(torch.uint8)
    actions_out.fill_(HOLD)
    actions_out[env] = store.action[f]
    fed.zero_()
    fed[env] = 1


def replay_judge(fed, done, reward64, job, pos, offset, played, done_at, return64, claim, job_demo, job_seeds, ids_out, seeds_out, counters):
    """Behind that step (bbai_demo_replay_judge): fed envs ONLY -- a held env's done / reward64 are stale, a reseeded env's done reads 1 until its
    first real step -- advance pos; with done set the demo's done_at = played = pos and return64 = the env's reward64; with the demo used up
    and no done, played = pos, done_at = 0, return64 = 0; either way job = -1 (waiting).  `claim`: every env with job < 0 then takes the next
    position k of the job list (job_demo int32[J], job_seeds int64[J]): job = job_demo[k], pos = 0, ids_out[i] = i, seeds_out[i] =
    job_seeds[k] while k < J, ids_out[i] = -1 for every env that took nothing; without `claim`, ids_out / seeds_out are left alone.  counters
    int64[2] = the job cursor (in / out, may pass J) and the demos finished (running total).  ROCm tensors: k_demo_replay_judge, which hands
    positions out wave by wave in the order the waves arrive; host tensors: the same in torch ops, positions in env order."""
    import torch
    n, D, J = int(job.shape[0]), int(offset.shape[0]) - 1, int(job_seeds.shape[0])
    if fed.is_cuda:
        assert fed.shape[0] == done.shape[0] == reward64.shape[0] == pos.shape[0] == ids_out.shape[0] == seeds_out.shape[0] == n
        assert played.shape[0] == done_at.shape[0] == return64.shape[0] == D and job_demo.shape[0] == J and counters.shape[0] == 2
        _launch("bbai_demo_replay_judge", n, (fed, torch.uint8), (done, torch.uint8), (reward64, torch.float64), (job, torch.int32), (pos, torch.int32),
                D, (offset, torch.int64), (played, torch.int32), (done_at, torch.int32), (return64, torch.float64), 1 if claim else 0,
                (job_demo, torch.int32), (job_seeds, torch.int64), J, (ids_out, torch.int64), (seeds_out, torch.int64), (counters, torch.int64))
        return counters
    env = ((fed != 0) & (job >= 0) & (job < D)).nonzero().reshape(-1)
    pos[env] += 1
    d, p = job[env].to(torch.int64), pos[env]
    dn = done[env] != 0
    end = dn | (p >= offset[d + 1] - offset[d])
    env, d, p, dn = env[end], d[end], p[end], dn[end]
    played[d] = p
    done_at[d] = torch.where(dn, p, torch.zeros_like(p))
    return64[d] = torch.where(dn, reward64[env], torch.zeros_like(reward64[env]))
    job[env] = -1
    counters[1] += len(env)
    if claim:
        free = (job < 0).nonzero().reshape(-1)
        k = int(counters[0]) + torch.arange(len(free))
        got, k = free[k < J], k[k < J]
        ids_out.fill_(-1)
        ids_out[got] = got
        seeds_out[got] = job_seeds[k]
        job[got] = job_demo[k]
        pos[got] = 0
        counters[0] += len(free)
    return counters


class DemoReplay(object):
    """What `DemoStore.replay` found, per demo, on the store's device and in the store's order: played int32 (actions of the demo that were
    applied; below the length iff the episode ended early), done_at int32 (the number of actions after which `done` arrived; 0 = not within
    the demo), return64 float64 (the env's reward of that step, bit for bit; 0.0 with done_at == 0), mismatches int32 (played frames whose
    (image, direction) differ from the recorded ones), first_mismatch int32 (the first such frame, -1 = none), mission_ok uint8 (the env's
    token row at frame 0 equals the store's); `length` int32 and `seeds` (uint64 on the host) as given."""

    def __init__(self, played, done_at, return64, mismatches, first_mismatch, mission_ok, length, seeds):
        self.played, self.done_at, self.return64 = played, done_at, return64
        self.mismatches, self.first_mismatch, self.mission_ok = mismatches, first_mismatch, mission_ok
        self.length, self.seeds = length, seeds

    def __len__(self):
        return int(self.played.shape[0])

    @property
    def exact(self):
        """The demo is the engine's episode of its seed, frame for frame and to its end."""
        return (self.done_at == self.length) & (self.mismatches == 0) & (self.mission_ok != 0)

    def logs(self):
        """The shape `evaluate` logs (babyai/evaluate.py:40-46)."""
        return {"num_frames_per_episode": self.played.cpu().tolist(), "return_per_episode": self.return64.cpu().tolist(),
                "seed_per_episode": [int(s) for s in self.seeds]}


def _replay(store, env_name, seeds, device, pool, reseed_every, poll_every, env):
    """`DemoStore.replay`.  The D' non-empty demos are the jobs, in the store's order; P = min(pool, D') envs (auto_reset=False, HOLD on, token
    rows on) start on the first P of them.  One tick: replay_feed (compare, hand out the recorded actions, HOLD for the rest), env.step,
    replay_judge (score the fed envs; on every r-th tick the free envs claim the next jobs) and, on those ticks, env.reseed(ids_out,
    seeds_out, levels=1) with the device lists the judge wrote -- no host data hands out work.  The host reads the two counters every
    `poll_every` ticks and stops at finished == D'; once the cursor has passed D' nothing can be claimed and the claims and reseeds stop."""
    import torch
    from .engine import seeds_u64
    seeds_h = seeds_u64(seeds, "replay")
    D = len(store)
    if len(seeds_h) != D:
        raise ValueError("replay: %d seeds for %d demonstrations" % (len(seeds_h), D))
    r = REPLAY_RESEED_EVERY if reseed_every is None else int(reseed_every)
    poll = int(poll_every)
    if r < 1 or poll < 1 or (env is None and int(pool) < 1):
        raise ValueError("replay: pool, reseed_every and poll_every must be at least 1")
    lens = store.lengths
    jobs_h = np.flatnonzero(lens > 0).astype(np.int32)
    J = len(jobs_h)
    dev = store.device
    i32 = dict(dtype=torch.int32, device=dev)
    played, done_at, mismatches = torch.zeros(D, **i32), torch.zeros(D, **i32), torch.zeros(D, **i32)
    first_mismatch = torch.full((D,), -1, **i32)
    return64 = torch.zeros(D, dtype=torch.float64, device=dev)
    mission_ok = torch.zeros(D, dtype=torch.uint8, device=dev)
    rep = DemoReplay(played, done_at, return64, mismatches, first_mismatch, mission_ok, torch.as_tensor(lens.astype(np.int32), device=dev), seeds_h)
    if J == 0:
        return rep
    job_seeds_h = seeds_h[jobs_h]
    own = env is None
    if own:
        from .engine import BatchedBabyAIEnv
        P = min(int(pool), J)
        env = BatchedBabyAIEnv(env_name, P, device=device, seeds=job_seeds_h[:P], auto_reset=False)
    hold_before = None
    try:
        P = int(env.num_envs)
        if torch.device(env.device) != dev:
            raise ValueError("replay: the store is on %s, the pool on %s" % (dev, env.device))
        if P > J:
            raise ValueError("replay: %d envs for %d non-empty demonstrations" % (P, J))
        if getattr(env, "done_actions", False):
            raise ValueError("replay: the pool is in the reference's done-action mode; a store does not say whether a recorded `done` was the "
                             "enum member, so such a replay is undefined")
        if own:
            env.enable_instr_tokens()
            env.reset()
        if hasattr(env, "set_option"):
            hold_before = env.get_option("step_hold")
            env.set_option("step_hold", 1)
        job_demo = torch.as_tensor(jobs_h, device=dev)
        job_seeds = torch.as_tensor(job_seeds_h.view(np.int64), device=dev)
        job, pos = job_demo[:P].clone(), torch.zeros(P, **i32)
        actions, fed = torch.full((P,), HOLD, dtype=torch.uint8, device=dev), torch.zeros(P, dtype=torch.uint8, device=dev)
        ids_out, seeds_out = torch.full((P,), -1, dtype=torch.int64, device=dev), torch.zeros(P, dtype=torch.int64, device=dev)
        counters = torch.as_tensor(np.array([P, 0], dtype=np.int64), device=dev)
        budget = (-(-J // P) + 1) * (int(lens.max()) + r) + poll
        tick, claiming = 0, P < J
        while True:
            if tick >= budget:
                raise RuntimeError("replay: %d ticks and not every demonstration finished (a pool that never reports `done`?)" % tick)
            with _Timed(dev, "feed"):
                replay_feed(env.image, env.direction, env.instr, job, pos, store, mismatches, first_mismatch, mission_ok, actions, fed)
            with _Timed(dev, "step"):
                env.step(actions)
            tick += 1
            claim = claiming and tick % r == 0
            with _Timed(dev, "judge"):
                replay_judge(fed, env.done, env.reward64, job, pos, store.offset, played, done_at, return64, claim, job_demo, job_seeds,
                             ids_out, seeds_out, counters)
            if claim:
                with _Timed(dev, "reseed"):
                    env.reseed(ids_out, seeds_out, levels=1)
            if tick % poll == 0:
                c = counters.cpu().numpy()                                      # 16 bytes: the loop's one synchronisation
                if int(c[1]) >= J:
                    break
                claiming = claiming and int(c[0]) < J
        return rep
    finally:
        if hold_before is not None and hold_before != 1:
            env.set_option("step_hold", hold_before)
        if own:
            env.close()


def grow_training_set(store, policy, env_name, eval_seed, grow_factor, num_eval_demos, device="cuda:0", pixel=False, pool=None, max_rounds=64,
                      reseed_levels=None):
    """`grow_training_set` of scripts/train_intelligent_expert.py:150-176, step for step: until `store` holds int(len(store) * grow_factor)
    demonstrations, evaluate `policy` (a tensor policy of `evaluate.evaluate_policy`) on num_eval_demos fresh seeds from eval_seed on (:158-160),
    move eval_seed past them (:166), take the seeds of the episodes with return <= 0 in episode order, cut to the number still missing
    (:162-165, :168), have the expert make one demonstration for each (`DemoStore.collect_seeds`, :169) and extend the store (:171).  Returns
    the new eval_seed (:176).  `pool`: the env pool of both the evaluation and the collection (None: one env per evaluation episode, the
    default pool of collect_seeds).  The reference loops for ever under a learner that never fails -- or whose failures the expert cannot
    solve either; here `max_rounds` evaluations in a row that add nothing raise RuntimeError.  `reseed_levels`: the depth of the reseeds of
    both (evaluate_policy with a pool, collect_seeds); both play one episode per seed, so 1 changes no result."""
    from .evaluate import evaluate_policy
    target = int(len(store) * grow_factor)
    idle = 0
    while len(store) < target:
        logs = evaluate_policy(policy, env_name, eval_seed, num_eval_demos, pixel=pixel, device=device, pool=pool,
                               **({} if pool is None or reseed_levels is None else {"reseed_levels": reseed_levels}))
        eval_seed += num_eval_demos
        fail = [s for s, r in zip(logs["seed_per_episode"], logs["return_per_episode"]) if r <= 0][:target - len(store)]
        before = len(store)
        if fail:
            new, _ = DemoStore.collect_seeds(env_name, fail, device=device, **({} if pool is None else {"pool": pool}),
                                             **({} if reseed_levels is None else {"reseed_levels": reseed_levels}))
            store.extend(new)
        idle = 0 if len(store) > before else idle + 1
        if idle >= max_rounds:
            raise RuntimeError("grow_training_set: %d evaluations in a row added no demonstration" % idle)
    return eval_seed


def run_batch(acmodel, batch, recurrence, entropy_coef, optimizer=None):
    """`ImitationLearning.run_epoch_recurrence_one_batch` (imitation.py:225-321) over a DemoBatch: the same two phases, the model
    called the same way, the same log.  `optimizer` given = a training batch (is_training)."""
    import torch
    dev = batch.image.device
    B, F = len(batch), batch.num_frames
    memories = torch.zeros([F, acmodel.memory_size], device=dev)
    memory = torch.zeros([B, acmodel.memory_size], device=dev)
    instr_embedding = acmodel._get_instr_embedding(batch.instr)
    # phase 1: the memories of every frame, no gradient; step t visits the demos that have a frame t
    for t in range(int(batch.lengths[0])):
        c = int(batch.counts[t])
        idx = batch.active(t)
        obs = TensorDict(image=batch.image[idx].to(torch.float32), instr=batch.instr[:c])
        with torch.no_grad():
            new_memory = acmodel(obs, memory[:c, :], instr_embedding[:c])["memory"]
        memories[idx, :] = memory[:c, :]
        memory[:c, :] = new_memory
    # phase 2: back-propagation through `recurrence` steps from every starting index
    final_loss, final_entropy, final_policy_loss = 0, 0, 0
    indexes = batch.starting_indexes(recurrence)
    memory = memories[indexes]
    total_frames = len(indexes) * recurrence
    hits = []
    for _ in range(recurrence):
        ep = batch.episode_ids[indexes]
        obs = TensorDict(image=batch.image[indexes].to(torch.float32), instr=batch.instr[ep])
        action_step = batch.action[indexes]
        res = acmodel(obs, memory * batch.mask[indexes], instr_embedding[ep])
        dist, memory = res["dist"], res["memory"]
        entropy = dist.entropy().mean()
        policy_loss = -dist.log_prob(action_step).mean()
        loss = policy_loss - entropy_coef * entropy
        action_pred = dist.probs.max(1, keepdim=True)[1]
        hits.append((action_pred == action_step.unsqueeze(1)).sum())
        final_loss += loss
        final_entropy += entropy
        final_policy_loss += policy_loss
        indexes = indexes + 1
    final_loss /= recurrence
    if optimizer is not None:
        optimizer.zero_grad()
        final_loss.backward()
        optimizer.step()
    accuracy = 0
    for h in torch.stack(hits).cpu().tolist():                   # (one read for all steps; summed as the reference sums them)
        accuracy += float(h) / total_frames
    return {"entropy": float((final_entropy / recurrence).detach()), "policy_loss": float((final_policy_loss / recurrence).detach()),
            "accuracy": float(accuracy)}


def run_epoch(acmodel, store, indices, batch_size, recurrence, entropy_coef, optimizer=None, vocab=None):
    """`run_epoch_recurrence` (imitation.py:189-223): batches of `batch_size` demos taken from `indices` in order (a shuffled
    permutation for training), a trailing partial batch dropped.  Without an optimizer the model is put in eval mode for the epoch."""
    batch_size = min(batch_size, len(store))
    if optimizer is None:
        acmodel.eval()
    log = {"entropy": [], "policy_loss": [], "accuracy": []}
    frames = 0
    for b in range(len(indices) // batch_size):
        batch = store.batch(indices[b * batch_size:(b + 1) * batch_size], vocab=vocab)
        frames += batch.num_frames
        one = run_batch(acmodel, batch, recurrence, entropy_coef, optimizer)
        for k in log:
            log[k].append(one[k])
    log["total_frames"] = frames
    if optimizer is None:
        acmodel.train()
    return log
