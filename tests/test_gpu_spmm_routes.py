"""Every kernel of csrc/spmm.hip at the smallest shape that reaches it: each case first asks kgcn_spmm_route_query which kernel
its call takes -- so a moved threshold fails here instead of silently testing another kernel -- then makes the call through the
public entry point and compares with the fp64 numpy product of oracle/kgcn_oracle.py (kgcn/layers.py:105-116, kgcn/bspmm_call.py:45,
kgcn/bconv_call.py:11-23 / :45-53, kgcn/layers.py:461-472)."""
import numpy as np
import pytest
import torch

from test_gpu_parity import K, close, dev, t32

pytestmark = pytest.mark.gpu
DACT, SELF, DOT, FANOUT = 1, 2, 4, 8
T = 3


def _mols(rng, n, channels=1):
    """adjs[b][c]: molecule-like graphs of n nodes (~3 entries per row) with random values"""
    adjs = []
    for _ in range(T):
        row = []
        for _ in range(channels):
            idx, val, shape = K.synth_mol_graphs(rng, 1, n, 3)[0][0]
            row.append((np.asarray(idx, np.int32), (np.asarray(val) * rng.standard_normal(len(val))).astype(np.float32), [n, n]))
        adjs.append(row)
    return adjs


def _expect(got, kernel, targs):
    assert (got[0], got[1][:len(targs)]) == (kernel, list(targs)), "the call takes %s<%s>, this case is about %s<%s>" % (
        got[0], got[1], kernel, list(targs))


@pytest.mark.parametrize("n,d,kernel,targs", [
    (10, 32, "spmm_tile", (8, 4, 1, 0)),
    (10, 50, "spmm_tile", (32, 2, 1, 0)),          # even width that is no multiple of 4: 8-byte vectors
    (50, 256, "spmm_tile", (64, 4, 4, 0)),         # a 51 KB tile: four waves, and more than 64 KB of LDS allowed for the kernel
    (20, 64, "spmm_slices", (2,)),
    (20, 128, "spmm_slices", (4,)),
    (10, 7, "spmm_gather", (1,)),                  # odd width: no vectors
])
def test_single_channel_batches(n, d, kernel, targs):
    from kgcn_amd import _lib
    from kgcn_amd.batched_csr import BatchedAdjacency
    rng = np.random.default_rng(n * 1000 + d)
    adjs = _mols(rng, n)
    a = BatchedAdjacency.from_adjs(adjs, n_nodes=n, device=dev()).channels[0]
    _expect(_lib.spmm_route(a.desc(), 1, d, d, n * d, 0, d, n * d), kernel, targs)
    x = rng.standard_normal((T, n, d)).astype(np.float32)
    out = torch.full((T * n, d), 7.0, device=dev())
    tx = t32(x.reshape(T * n, d))
    _lib.check(_lib.lib.kgcn_bspmm_f32(a.desc(), _lib.ptr(tx), d, n * d, d, _lib.ptr(out), d, n * d, 0.0, _lib.current_stream()))
    ref = np.concatenate(K.bspmm([row[0] for row in adjs], list(x)))
    close(out, ref, rel=2e-6, what="%s<%s>" % (kernel, targs))


def test_gin_backward_with_d_epsilon_takes_the_dot_form_of_the_tile_kernel():
    from kgcn_amd import _lib
    from kgcn_amd.batched_csr import BatchedAdjacency
    n, d = 10, 32
    rng = np.random.default_rng(5)
    adjs = _mols(rng, n)
    adj = BatchedAdjacency.from_adjs(adjs, n_nodes=n, device=dev())
    at = adj.desc_array(True)
    _expect(_lib.spmm_route(at, 1, d, d, n * d, 0, d, n * d, flags=SELF | DOT), "spmm_tile_dot", (8, 4, 1, 1))
    g = rng.standard_normal((T, n, d)).astype(np.float32)
    x = rng.standard_normal((T, n, d)).astype(np.float32)
    tg, tx, eps = t32(g.reshape(-1, d)), t32(x.reshape(-1, d)), t32(np.array([0.37]))
    dx = torch.full((T * n, d), 7.0, device=dev())
    deps = torch.full((1,), 7.0, device=dev())
    wsb = _lib.lib.kgcn_gin_aggregate_bwd_workspace_bytes(T, n, d)
    ws = _lib.workspace(wsb, dev())
    _lib.check(_lib.lib.kgcn_gin_aggregate_bwd_f32(at, 1, _lib.ptr(tg), d, _lib.ptr(eps), _lib.ptr(tx), _lib.ptr(dx), _lib.ptr(deps),
                                                   _lib.ptr(ws), wsb, _lib.current_stream()))
    ref = np.concatenate([np.float64(np.float32(0.37)) * gb + K.spmm_coo(row[0], gb, adjoint_a=True) for row, gb in zip(adjs, g)])
    close(dx, ref, rel=2e-6, what="GIN backward dx (tile DOT)")
    close(deps, np.array([(g.astype(np.float64) * x).sum()]), rel=2e-6, what="GIN backward d eps (tile DOT)")


def test_two_channels_take_the_channel_loop_forward_and_its_fan_out_backward():
    from kgcn_amd import _lib
    from kgcn_amd.batched_csr import BatchedAdjacency
    n, d, C = 10, 32, 2
    rng = np.random.default_rng(6)
    adjs = _mols(rng, n, C)
    adj = BatchedAdjacency.from_adjs(adjs, n_nodes=n, device=dev())
    _expect(_lib.spmm_route(adj.desc_array(), C, d, C * d, n * C * d, d, d, n * d), "bconv_loop", (4, 8, 8))
    _expect(_lib.spmm_route(adj.desc_array(True), C, d, d, n * d, d, C * d, n * C * d, flags=FANOUT), "bconv_fanout", (4, 8))
    rhs = rng.standard_normal((T * n, C * d)).astype(np.float32)
    g = rng.standard_normal((T * n, d)).astype(np.float32)
    dense = [[rhs[b * n:(b + 1) * n, c * d:(c + 1) * d] for c in range(C)] for b in range(T)]
    trhs, tg = t32(rhs), t32(g)                      # (held in variables: a temporary's memory is reused by the next allocation)
    out = torch.full((T * n, d), 7.0, device=dev())
    _lib.check(_lib.lib.kgcn_bconv_f32(adj.desc_array(), C, _lib.ptr(trhs), C * d, n * C * d, d, d, _lib.ptr(out), d, n * d,
                                       _lib.current_stream()))
    close(out, np.concatenate(K.bconv(adjs, dense)), rel=2e-6, what="bconv_loop<4,8,8>")
    fan = torch.full((T * n, C * d), 7.0, device=dev())
    _lib.check(_lib.lib.kgcn_bconv_fanout_f32(adj.desc_array(True), C, _lib.ptr(tg), None, d, n * d, d, 0, _lib.ptr(fan), C * d,
                                              n * C * d, d, _lib.current_stream()))
    _, rg = K.bconv_grad(adjs, dense, [g[b * n:(b + 1) * n] for b in range(T)])
    close(fan, np.concatenate([np.concatenate(rg[b], axis=1) for b in range(T)]), rel=2e-6, what="bconv_fanout<4,8>")


@pytest.mark.parametrize("blocks", [True, False])
@pytest.mark.parametrize("dact", [0, 3])
def test_ragged_compact_batch_with_and_without_its_block_table(blocks, dact):
    """the block kernel with the table; the same container without it goes to the row-chunk kernel, two rows per lane group"""
    from kgcn_amd import _lib, ragged
    from kgcn_amd.batched_csr import BatchedCSR
    from test_oracle_model import tox21_like_batch
    rng = np.random.default_rng(8)
    x, adjs, _, _, _, sizes = tox21_like_batch(rng, B=60, N=12, F=3, T=2)
    rb = ragged.compact(t32(x), adjs, sizes)
    a = rb.adjacency.channels[0]
    if dact:
        a = a.transpose()
    if not blocks:
        a = BatchedCSR(a.rowptr, a.cv, a.num_graphs, a.rows, a.cols, a.max_nnz)
    R, d = rb.capacity, 32
    got = _lib.spmm_route(a.desc(), 1, d, d, R * d, 0, d, R * d, flags=DACT if dact else 0)
    if blocks:
        _expect(got, "spmm_block", (4, 8, 1 if dact else 0))
    else:
        _expect(got, "spmm_rows", (4, 16, 1 if dact else 0, 2))
    rp = a.rowptr.cpu().numpy().astype(np.int64)
    cv = a.cv.cpu().numpy()[:rp[-1]]
    coo = (np.stack([np.repeat(np.arange(R), np.diff(rp)), cv[:, 0]], 1), cv[:, 1].copy().view(np.float32), [R, R])
    g = rng.standard_normal((R, d)).astype(np.float32)
    ao = np.tanh(rng.standard_normal((R, d))).astype(np.float32)
    tg, tao = t32(g), t32(ao)                        # (held in variables: a temporary's memory is reused by the next allocation)
    out = torch.full((R, d), 7.0, device=dev())
    _lib.check(_lib.lib.kgcn_bspmm_dact_f32(a.desc(), _lib.ptr(tg), _lib.ptr(tao) if dact else None, d, R * d, d, dact,
                                            _lib.ptr(out), d, R * d, 0.0, _lib.current_stream()))
    ref = K.spmm_coo(coo, g.astype(np.float64) * ((1.0 - ao.astype(np.float64) ** 2) if dact else 1.0))
    close(out, ref, rel=2e-6, what="ragged-compact aggregation (%s)" % got[0])


def test_block_diagonal_batch_beyond_32768_rows_takes_eight_rows_per_lane_group():
    from kgcn_amd import _lib
    from kgcn_amd.batched_csr import BatchedCSR
    G, n, d = 3300, 10, 8
    rng = np.random.default_rng(9)
    rows, cols = [], []
    for b, row in enumerate(K.synth_ring_graphs(rng, G, n)):
        idx = np.asarray(row[0][0]).reshape(-1, 2)
        rows.append(idx[:, 0] + b * n)
        cols.append(idx[:, 1] + b * n)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.standard_normal(rows.size).astype(np.float32)
    R = G * n
    a = BatchedCSR.from_arrays(np.zeros(rows.size, np.int64), rows, cols, vals, 1, R, R, device=dev())
    _expect(_lib.spmm_route(a.desc(), 1, d, d, R * d, 0, d, R * d), "spmm_rows", (4, 16, 0, 8))
    x = rng.standard_normal((R, d)).astype(np.float32)
    tx = t32(x)
    out = torch.full((R, d), 7.0, device=dev())
    _lib.check(_lib.lib.kgcn_bspmm_f32(a.desc(), _lib.ptr(tx), d, R * d, d, _lib.ptr(out), d, R * d, 0.0, _lib.current_stream()))
    close(out, K.spmm_coo((np.stack([rows, cols], 1), vals, [R, R]), x), rel=2e-6, what="spmm_rows<4,16,0,8>")
