"""The dX stores of the FULL-shape fused GraphConv backward (N = 32, din = dout = 64).

The pairs kernel (T >= 2,048) computes dX = dFW W^T un-transposed -- lane = feature, register = node -- and stores every accumulator
register, behind one v_permlane32_swap, as ONE whole 256-byte row of dX; the planes kernel (T < 2,048) stores 32-byte segments of 32
rows per instruction.  Both write each element of dX exactly once and nothing else.  The backward entry point is called directly with
a dX that lies in the middle of a larger buffer: the whole buffer is pre-filled with one NaN bit pattern, every element of dX has to be
overwritten and no word of the guard regions in front of and behind it may change.  T = 1, 2, 3 are all prologue and epilogue;
2,047 / 2,048 / 2,049 straddle the switch between the two kernels; 4,000 gives the pairs three or four graphs; 100,000 is the
benchmark size.  Unit and Kipf-normalised adjacency values select the two value streams of the compact layout.

Reference (fp64 numpy) and tolerances are those of tests/test_gpu_fused_ingest.py; nothing is compared more loosely here.
"""
import numpy as np
import pytest
import torch

from oracle import kgcn_oracle as K
from test_gpu_parity import close, dev, t32

pytestmark = pytest.mark.gpu

N, D = 32, 64
GUARD = 4096                    # floats in front of and behind dX (16 KiB each: two tiles)
FILL = 0x7fc0a5a5               # a quiet NaN with a payload no kernel produces


@pytest.mark.parametrize("normalize", [False, True], ids=["unit", "kipf"])
@pytest.mark.parametrize("T", [1, 2, 3, 2047, 2048, 2049, 4000, 100000])
def test_dx_written_once_inside_guards(T, normalize):
    from kgcn_amd import BatchedCSR, _lib, ops
    from kgcn_amd._lib import check, current_stream, lib, ptr
    rng = np.random.default_rng(104729 * T + int(normalize))
    adjs = K.synth_mol_graphs(rng, T, N, 3, normalize=normalize)
    x = rng.standard_normal((T, N, D)).astype(np.float32)
    w = K.glorot_uniform(rng, D, D)
    g = rng.standard_normal((T, N, D)).astype(np.float32)
    csr = BatchedCSR.from_coo_list([a[0] for a in adjs], rows=N, cols=N, device=dev())
    assert ops.graphconv_fused_supported(csr, D, D)
    at = csr.transpose()
    p4t = at.padded4()
    pairs = lib.kgcn_graphconv_fused_reads_compact(1, T, p4t.rows, D, D, p4t.max_nnz, 1)
    assert bool(pairs) == (T >= 2048), "backward route for T = %d: pairs = %d" % (T, pairs)
    tx, tw, tg = t32(x), t32(w), t32(g)
    desc = ops._fused_adjacency(at, True, T, D, D, True)
    wsb = lib.kgcn_graphconv_bwd_workspace_bytes(T, D, D)
    wsp = _lib.workspace(wsb, dev())

    def launch():
        buf = torch.full((GUARD + T * N * D + GUARD,), FILL, dtype=torch.int32, device=dev())
        dx = buf[GUARD:GUARD + T * N * D].view(torch.float32).view(T, N, D)
        assert dx.data_ptr() == buf.data_ptr() + 4 * GUARD and dx.data_ptr() % 16 == 0
        dwb = torch.full((D * D + D,), float("nan"), dtype=torch.float32, device=dev())
        dw, db = dwb[:D * D].view(D, D), dwb[D * D:]
        check(lib.kgcn_graphconv_bwd_f32(desc, ptr(tx), ptr(tw), ptr(tg), D, D, ptr(dx), ptr(dw), ptr(db), ptr(wsp), wsb,
                                         current_stream()), "kgcn_graphconv_bwd_f32")
        torch.cuda.synchronize()
        return buf, dx, dw, db

    buf, dx, dw, db = launch()
    front, back = buf[:GUARD], buf[GUARD + T * N * D:]
    assert int((front != FILL).sum()) == 0, "%d words in front of dX were written" % int((front != FILL).sum())
    assert int((back != FILL).sum()) == 0, "%d words behind dX were written" % int((back != FILL).sum())
    left = buf[GUARD:GUARD + T * N * D] == FILL
    assert int(left.sum()) == 0, "%d elements of dX were not written (first at flat index %d)" % (
        int(left.sum()), int(torch.nonzero(left)[0]))
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
    rdx, rdw, rdb = K.graphconv_bwd_fast(x, adjs, [w], g)
    close(dx, rdx, rel=1e-6, what="fused dX")
    close(dw, rdw[0], rel=1e-5, what="fused dW")
    close(db.reshape(1, D), rdb[0], rel=1e-5, what="fused dbias")
    buf2, _, dw2, db2 = launch()
    assert torch.equal(buf, buf2), "dX (or a guard word) differs between two launches on the same operands"
    assert torch.equal(dw.view(torch.int32), dw2.view(torch.int32)), "dW differs between two launches"
    assert torch.equal(db.view(torch.int32), db2.view(torch.int32)), "dbias differs between two launches"
