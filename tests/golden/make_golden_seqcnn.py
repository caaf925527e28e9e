"""Writes tests/golden/g9_seqcnn.npz: a synthetic stand-in for the dataset.jbl of sample_protein/sequence/02make_dataset.py (the
sample's real sequences are downloaded by its 00get_fasta.py).  NumPy only.

  sequence             [G, L] int32, symbols 0..25 (ord(c) - ord('A')), every row padded with 0 to the longest one, as the script pads
  sequence_length      [G]
  label                [G, 2] one-hot; class 1 carries the planted motif MOTIF once at a random place, class 0 does not
  class_weight         sum(v) / v with v the class counts, as the script computes it
  sequence_symbol_num  max token + 1

    python tests/golden/make_golden_seqcnn.py
"""
import os

import numpy as np

G, LMIN, LMAX, SYMBOLS, POSITIVE_RATE = 240, 60, 96, 26, 0.3
MOTIF = np.array([22, 7, 22, 7, 24, 24, 22, 7], np.int32)


def make(seed=9):
    rng = np.random.default_rng(seed)
    labels = (rng.random(G) < POSITIVE_RATE).astype(np.int64)
    lengths = rng.integers(LMIN, LMAX + 1, size=G)
    lengths[0] = LMAX
    seq = np.zeros((G, LMAX), np.int32)
    for i in range(G):
        s = rng.integers(0, SYMBOLS, size=lengths[i]).astype(np.int32)
        s[s == 22] = 3                                   # the motif's leading symbol occurs nowhere else
        if labels[i]:
            at = int(rng.integers(0, lengths[i] - len(MOTIF) + 1))
            s[at:at + len(MOTIF)] = MOTIF
        seq[i, :lengths[i]] = s
    label = np.zeros((G, 2), np.float32)
    label[np.arange(G), labels] = 1.0
    v = label.sum(axis=0)
    return dict(sequence=seq, sequence_length=lengths.astype(np.int32), label=label, class_weight=(v.sum() / v).astype(np.float64),
                sequence_symbol_num=np.int32(seq.max() + 1))


if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g9_seqcnn.npz")
    np.savez_compressed(out, **make())
    print(out, os.path.getsize(out), "bytes")
