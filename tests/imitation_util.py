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
