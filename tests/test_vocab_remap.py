"""A reference-trained model's vocabulary on the tensor fast path: the reference's own `InstructionsPreprocessor`
(babyai/utils/format.py:44-75, ids in first-seen order, saved as vocab.json) against the engine's fixed token ids pushed
through `babyai_amd.preprocess.remap_table` -- on 10^4 missions drawn from every level.  What the reference's preprocessor made of
them (the vocabulary it saved, its token ids) is recorded by tools/gen_golden_refpin.py in tests/golden/refpin/vocab.npz."""
import json

import numpy as np

from babyai_amd.missions import tokenize
from babyai_amd.preprocess import remap_table
import refpin_util as rp


def test_remap_table_reproduces_the_reference_preprocessor():
    with np.load(rp.golden_path("vocab.npz")) as f:
        g = {k: f[k] for k in f.files}
    missions = rp.vocab_missions()
    assert rp.missions_digest(missions) == str(g["missions_sha256"]), "the missions are not the ones the record was taken on"
    # a "trained model": its vocabulary grew in first-seen order over the first 300 missions only
    vocab = json.loads(str(g["trained_vocab"]))
    assert 5 < len(vocab) <= 32
    lut, extended = remap_table(vocab)
    assert all(extended[w] == vocab[w] for w in vocab)
    # the reference preprocessor, continuing from the saved vocabulary, on all 10^4 missions in one batch per 500
    assert len(g["ids"]) == len(missions)
    for row, m in zip(g["ids"], missions):
        ids = [lut[t] for t in tokenize(m)]
        assert list(row[:len(ids)]) == ids and not row[len(ids):].any(), m
    # a vocabulary that has seen only a few words: known words keep their ids exactly, unseen ones get the next free
    # ids (distinct, above the loaded ones), as Vocabulary.__getitem__ would hand them out
    v2 = json.loads(str(g["small_vocab"]))
    assert len(v2) < 12
    lut2, ext2 = remap_table(v2)
    assert all(ext2[w] == v2[w] for w in v2)
    new_ids = sorted(ext2[w] for w in ext2 if w not in v2)
    assert new_ids == list(range(len(v2) + 1, 33)) and len(set(lut2[1:])) == 32
    known_only = [m for m in missions if all(w in v2 for w in m.replace(",", " ").split())]
    assert known_only
    assert list(g["known_only"]) == known_only[:200]
    for row, m in zip(g["again_ids"], known_only[:200]):
        ids = [lut2[t] for t in tokenize(m)]
        assert list(row[:len(ids)]) == ids and not row[len(ids):].any(), m
