"""No bit of a loss or metric moves: every head that sums over a workgroup (csrc/block_reduce.h: block_sum, the shared finish
kernel) replays the inputs of tests/golden/reduction_bits.npz and must return the stored bits -- sums / stats, the gradient with
respect to the logits, predictions and the accumulator block after two calls.  The fixture was recorded with the library as it
was before those sums were gathered into one header (tests/golden/make_golden_reduction_bits.py lists the cases)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_reduction_bits as G  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(G.PATH, allow_pickle=False)


@pytest.mark.parametrize("name,head,p", G.CASES, ids=[c[0] for c in G.CASES])
def test_bits_are_the_stored_ones(golden, name, head, p):
    import torch
    pre_in, pre_out = name + "/in_", name + "/out_"
    inp = {k[len(pre_in):]: golden[k] for k in golden.files if k.startswith(pre_in)}
    want = {k[len(pre_out):]: golden[k] for k in golden.files if k.startswith(pre_out)}
    got = G.run(head, p, inp)
    assert sorted(got) == sorted(want) and want
    for k, v in got.items():
        w = torch.from_numpy(want[k].view(np.int32))
        differ = int((v != w).sum()) if v.shape == w.shape else -1
        print("%-28s %-8s %d words, %d differ" % (name, k, w.numel(), differ))
        assert torch.equal(v, w), (name, k, differ)
