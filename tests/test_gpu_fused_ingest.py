"""The FULL-shape fused GraphConv kernels (N = 32, din = dout = 64) at the batch sizes where their software pipelines begin and end.

The forward streams x in and the output out with a streaming (nontemporal) cache policy, one graph ahead of the contraction; the
backward keeps two graphs in flight per wave (planes kernel, T < 2,048) or per pair of waves (pairs kernel, T >= 2,048).  T = 1, 2, 3
are all prologue and epilogue; 2,047 / 2,048 / 2,049 straddle the switch between the two backward kernels (every pair owns exactly
two graphs / one pair owns three); 4,000 gives the pairs three or four graphs and the forward a ragged last step.  Both adjacency
value streams of the compact layout are exercised: unit values (no value stream) and Kipf-normalised values.

Tolerances are those of test_graphconv_fused (tests/test_gpu_parity.py); nothing is compared more loosely here.
"""
import numpy as np
import pytest
import torch

from oracle import kgcn_oracle as K
from test_gpu_parity import close, dev, t32

pytestmark = pytest.mark.gpu

N, D = 32, 64


@pytest.mark.parametrize("normalize", [False, True], ids=["unit", "kipf"])
@pytest.mark.parametrize("T", [1, 2, 3, 2047, 2048, 2049, 4000])
def test_full_shape_pipeline_edges(T, normalize):
    from kgcn_amd import BatchedCSR, ops
    rng = np.random.default_rng(7919 * T + int(normalize))
    adjs = K.synth_mol_graphs(rng, T, N, 3, normalize=normalize)
    x = rng.standard_normal((T, N, D)).astype(np.float32)
    w = K.glorot_uniform(rng, D, D)
    b = rng.standard_normal((1, D)).astype(np.float32)
    g = rng.standard_normal((T, N, D)).astype(np.float32)
    csr = BatchedCSR.from_coo_list([a[0] for a in adjs], rows=N, cols=N, device=dev())
    assert ops.graphconv_fused_supported(csr, D, D)
    # the cases straddle the switch between the two backward kernels only while the launcher's rule puts it at 2,048 graphs
    from kgcn_amd._lib import lib
    p4t = csr.transpose().padded4()
    pairs = lib.kgcn_graphconv_fused_reads_compact(1, T, p4t.rows, D, D, p4t.max_nnz, 1)
    assert bool(pairs) == (T >= 2048), "backward route for T = %d: pairs = %d" % (T, pairs)

    def launch():
        tx, tw, tb = t32(x).requires_grad_(True), t32(w).requires_grad_(True), t32(b).requires_grad_(True)
        out = ops.graphconv_fused(tx, tw, tb, csr)
        out.backward(t32(g))
        return out.detach(), tx.grad, tw.grad, tb.grad

    out, dx, dw, db = launch()
    ref = K.graphconv_fwd_fast(x, adjs, [w], [b])
    rdx, rdw, rdb = K.graphconv_bwd_fast(x, adjs, [w], g)
    close(out, ref, rel=1e-6, what="fused fwd")
    close(dx, rdx, rel=1e-6, what="fused dX")
    close(dw, rdw[0], rel=1e-5, what="fused dW")
    close(db, rdb[0], rel=1e-5, what="fused dbias")
    for first, again, name in zip((out, dx, dw, db), launch(), ("output", "dX", "dW", "dbias")):
        assert torch.equal(first, again), "%s differs between two launches on the same operands" % name
