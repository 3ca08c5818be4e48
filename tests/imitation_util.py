"""Test double for tests/test_imitation_*.py and tools/gen_golden_imitation.py: an actor-critic with the call contract
babyai/imitation.py uses (`memory_size`, `_get_instr_embedding(instr)`, `model(obs, memory, instr_embedding)` -> dist / memory)
whose arithmetic is EXACT in float32 -- small integers times multiples of 1/8 -- so that results do not depend on the order of a
sum, on the instruction padding width, or on whether a CPU or a GPU computed them.  The golden cases keep every mean over a power
of two of frames and use recurrences 1, 2 and 4, so the losses, the gradients and one SGD step with a power-of-two rate are exact
as well (the recording tool proves it by repeating every case in float64)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imitation")
LEVELS = ("GoToObjS4", "GoToLocalS5N2")
ENTROPY_COEF = 1.0 / 64
LR = 1.0 / 16
TOK_MAX = 72


class _Emb(torch.Tensor):
    """The reference indexes the instruction embedding with a float numpy array (imitation.py:250,295), which current torch
    refuses: this tensor takes such an index as the integers it holds."""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    def __getitem__(self, index):
        if isinstance(index, np.ndarray) and index.dtype.kind == "f":
            index = torch.as_tensor(index.astype(np.int64))
        return torch.Tensor.__getitem__(self.as_subclass(torch.Tensor), index)


class ToyDist(object):
    def __init__(self, scores):
        self.scores = scores
        self.probs = scores + torch.arange(7, device=scores.device, dtype=scores.dtype) / 64      # (no ties: scores are multiples of 1/8)

    def entropy(self):
        return (self.scores * self.scores).sum(1) / 64

    def log_prob(self, action):
        return self.scores.gather(1, action.unsqueeze(1)).squeeze(1) - self.scores.sum(1) / 8


class ToyILModel(torch.nn.Module):
    memory_size = 4

    def __init__(self, dtype=torch.float32, reference_indexing=False):
        super().__init__()
        w = (np.arange(35).reshape(7, 5) * 5 % 17 - 8) / 8.0
        self.weight = torch.nn.Parameter(torch.as_tensor(w, dtype=dtype))
        self.dtype, self.reference_indexing = dtype, reference_indexing
        self.calls = None                       # a list: every forward() appends what it was called with

    def _get_instr_embedding(self, instr):
        pos = torch.arange(1, instr.shape[1] + 1, device=instr.device)
        emb = torch.stack([instr.sum(1) % 4, (instr * pos).sum(1) % 4], dim=1).to(self.dtype)
        return _Emb(emb) if self.reference_indexing else emb

    def forward(self, obs, memory, instr_embedding):
        memory, emb = memory.to(self.dtype), torch.as_tensor(instr_embedding).as_subclass(torch.Tensor).to(self.dtype)
        if self.calls is not None:
            instr = np.zeros((obs.instr.shape[0], TOK_MAX), dtype=np.int16)
            instr[:, :obs.instr.shape[1]] = obs.instr.cpu().numpy()
            self.calls.append({"image": obs.image.detach().cpu().numpy().astype(np.uint8), "instr": instr,
                               "memory": memory.detach().cpu().numpy().astype(np.float32), "emb": emb.detach().cpu().numpy().astype(np.float32)})
        n = obs.image.shape[0]
        total = obs.image.reshape(n, -1).to(torch.int64).sum(1)
        words = obs.instr.reshape(n, -1).sum(1)
        x = torch.stack([(total % 4).to(self.dtype), emb[:, 0], emb[:, 1], memory[:, 0] % 4, torch.ones(n, device=total.device, dtype=self.dtype)], dim=1)
        scores = x @ self.weight.t()
        mem = ((memory[:, :1] + ((total % 5) + (words % 3) + 1).to(self.dtype).unsqueeze(1) + emb[:, :1]) % 8).expand(n, self.memory_size).clone()
        return {"dist": ToyDist(scores), "memory": mem, "value": scores[:, 0], "extra_predictions": {}}


def load_demos(level):
    """The recorded demonstrations of a level as the reference's tuples (images plain)."""
    with np.load(os.path.join(GOLDEN, "demos_%s.npz" % level)) as f:
        ends = np.cumsum(f["length"])
        return [(str(f["mission"][k]), f["image"][ends[k] - f["length"][k]:ends[k]], f["direction"][ends[k] - f["length"][k]:ends[k]].tolist(),
                 f["action"][ends[k] - f["length"][k]:ends[k]].tolist()) for k in range(len(ends))]


def strip(instr):
    """Token rows without their zero padding (the padding width is the caller's business)."""
    return [tuple(int(t) for t in row if t) for row in np.asarray(instr)]


# ------------------------------------------------------------------------------------------
# Synthetic inputs and plain references for k_demo_pack / k_demo_batch (tests/test_gpu_demo_kernels.py).  Everything here is numpy on
# the host: the cases are built, and their references computed, once per module and shared by the tests that use them.
# ------------------------------------------------------------------------------------------
ROW = 147                       # bytes of one 7x7x3 frame
BLOCK_BYTES = 8192              # bytes of the image array that one block of either kernel writes
HIST_KEYS = ("image", "direction", "action", "tokens")      # the order of include/bbai.h bbai_demo_chunk


def random_bytes(rng, *shape):
    """Independent random bytes: a misaddressed byte is wrong with probability 255/256."""
    return rng.integers(0, 256, size=shape, dtype=np.uint8)


def runs_per_block(start):
    """How many runs (demos) each 8 KiB block of an image array meets; start = int64[count + 1], first frame of each run and the
    frame count behind the last."""
    start = np.asarray(start, dtype=np.int64)
    total = int(start[-1]) * ROW
    out = []
    for byte0 in range(0, total, BLOCK_BYTES):
        first, last = byte0 // ROW, (min(byte0 + BLOCK_BYTES, total) - 1) // ROW
        out.append(int(np.searchsorted(start, last, side="right") - np.searchsorted(start, first, side="right")) + 1)
    return out


def blocks_inside_one_run(start):
    """Full 8 KiB blocks whose every byte belongs to one run."""
    total = int(np.asarray(start)[-1]) * ROW
    return sum(1 for b, runs in enumerate(runs_per_block(start)) if runs == 1 and (b + 1) * BLOCK_BYTES <= total)


class PackCase(object):
    """A history of C chunks of T steps of n streams, one span per stream, and what k_demo_pack must make of them."""

    def __init__(self, rng, T, C, n, lens, first=None):
        lens = np.asarray(lens, dtype=np.int64)
        assert lens.shape == (n,) and lens.min() >= 1 and lens.max() <= T * C
        if first is None:
            first = rng.integers(0, T * C - lens + 1)
        first = np.asarray(first, dtype=np.int64)
        assert first.min() >= 0 and (first + lens).max() <= T * C
        self.T, self.C, self.n = T, C, n
        self.span = np.stack([first, first + lens - 1], axis=1).astype(np.int32)
        self.offset = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.frames = int(self.offset[-1])
        self.hist = [{"image": random_bytes(rng, T, n, ROW), "direction": random_bytes(rng, T, n), "action": random_bytes(rng, T, n),
                      "tokens": random_bytes(rng, T, n, TOK_MAX)} for _ in range(C)]
        self.chunks_spanned = self.span[:, 1] // T - self.span[:, 0] // T + 1
        self.expect = pack_reference(self.hist, T, self.span, self.offset)
        for a in self.expect.values():
            a.setflags(write=False)


def pack_reference(hist, T, span, offset):
    """k_demo_pack in plain numpy: frame offset[k] + i of the store = history step g = span[k, 0] + i of stream k, which is row g % T of
    chunk g // T; the token row is that of the span's first step."""
    n, frames = len(span), int(offset[-1])
    image, direction = np.zeros((frames, ROW), np.uint8), np.zeros(frames, np.uint8)
    action, tokens = np.zeros(frames, np.uint8), np.zeros((n, TOK_MAX), np.uint8)
    for k in range(n):
        for i in range(int(span[k, 1]) - int(span[k, 0]) + 1):
            g = int(span[k, 0]) + i
            image[offset[k] + i] = hist[g // T]["image"][g % T, k]
            direction[offset[k] + i] = hist[g // T]["direction"][g % T, k]
            action[offset[k] + i] = hist[g // T]["action"][g % T, k]
        g = int(span[k, 0])
        tokens[k] = hist[g // T]["tokens"][g % T, k]
    return {"image": image, "direction": direction, "action": action, "tokens": tokens}


class SynthStore(object):
    """A store of random bytes with the given demo lengths (no tokens: neither k_demo_batch nor `imitation._gather` reads them)."""

    def __init__(self, rng, lens):
        self.lens = np.asarray(lens, dtype=np.int64)
        assert self.lens.min() >= 1
        self.offset = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.frames = int(self.offset[-1])
        self.image, self.direction, self.action = random_bytes(rng, self.frames, ROW), random_bytes(rng, self.frames), random_bytes(rng, self.frames)

    def __len__(self):
        return len(self.lens)


class BatchCase(object):
    """Demos `order` of a store laid end to end, and what k_demo_batch must make of them in both forms."""

    def __init__(self, store, order):
        self.store, self.order = store, np.ascontiguousarray(order, dtype=np.int64)
        assert self.order.ndim == 1 and self.order.size >= 1 and self.order.min() >= 0 and self.order.max() < len(store)
        self.dst_start = np.concatenate([[0], np.cumsum(store.lens[self.order])]).astype(np.int64)
        self.frames = int(self.dst_start[-1])
        self.expect = batch_reference(store.offset, self.order, self.dst_start, store.image, store.direction, store.action)
        for a in self.expect.values():
            a.setflags(write=False)


def batch_reference(offset, order, dst_start, src_image, src_dir, src_action):
    """k_demo_batch in plain numpy, both forms at once: frame dst_start[b] + i of the result = frame offset[order[b]] + i of the store."""
    frames = int(dst_start[-1])
    out = {"image": np.zeros((frames, ROW), np.uint8), "action": np.zeros(frames, np.int64), "done": np.zeros(frames, np.uint8),
           "mask": np.zeros(frames, np.float32), "episode": np.zeros(frames, np.int64), "dir8": np.zeros(frames, np.uint8),
           "action8": np.zeros(frames, np.uint8)}
    for b in range(len(order)):
        length = int(dst_start[b + 1] - dst_start[b])
        for i in range(length):
            s, f = int(offset[order[b]]) + i, int(dst_start[b]) + i
            out["image"][f] = src_image[s]
            out["action"][f] = src_action[s]
            out["dir8"][f] = src_dir[s]
            out["action8"][f] = src_action[s]
            out["done"][f] = i == length - 1
            out["mask"][f] = float(i != 0)
            out["episode"][f] = b
    return out
