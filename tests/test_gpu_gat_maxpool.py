"""The six GAT kernels (csrc/gat.hip) and the segmented-max pair (csrc/spmm.hip: maxpool_fwd_kernel, maxpool_bwd_kernel) against
the fp64 oracle on the directed, irregular cases of tests/layer_cases.py: full rows (max-pooling without the implicit zero),
referenced nodes that store nothing (GAT's denominator is 1e-10 alone), transposes that differ from the original in structure
and in values, second column trips, several nodes per workgroup of gat_bwd_dots_kernel, M != K.  tests/test_layer_cases.py shows
on the CPU that every case reaches what it names and which wrong kernels it would catch.

Tolerances are the ones tests/test_gpu_parity.py writes for the same tensors (test_gat_layer, test_graph_maxpooling)."""
import numpy as np
import pytest
import torch

import layer_cases as L
from test_gpu_parity import close, dev, t32

pytestmark = pytest.mark.gpu

GAT_CASES = [c for c in sorted(L.CASES) if L.CASES[c].get("gat", True)]


def _adjacency(d, adjs):
    """the packed batch of a case: through the layers' own packer where the adjacency is square"""
    from kgcn_amd import BatchedCSR
    from kgcn_amd.batched_csr import BatchedAdjacency
    if d["M"] == d["K"]:
        return BatchedAdjacency.from_adjs(adjs, n_nodes=d["M"], device=dev())
    return BatchedAdjacency([BatchedCSR.from_coo_list([a[c] for a in adjs], rows=d["M"], cols=d["K"], device=dev())
                             for c in range(d["C"])])


def _gat_run(d, adj):
    from kgcn_amd import layers
    layer = layers.GAT(d["C"]).to(dev())
    layer.build((d["T"], d["M"], d["D"]), dev())
    with torch.no_grad():
        for c in range(d["C"]):
            layer.weight_a[c].copy_(t32(d["weight_a"][c]))
    tx = t32(d["x"]).requires_grad_(True)
    out = layer(tx, adj=adj)
    out.backward(t32(d["g"]))
    return out.detach(), tx.grad, [w.grad for w in layer.weight_a]


@pytest.mark.parametrize("case", GAT_CASES)
def test_gat_against_the_fp64_oracle(case):
    d = L.make_case(case)
    ref = d["ref"]
    adj = _adjacency(d, d["adjs"])
    out, dx, dwa = _gat_run(d, adj)
    assert tuple(out.shape) == d["x"].shape
    for t in [out, dx] + dwa:
        assert bool(torch.isfinite(t).all())
    close(out, ref["gat_out"], atol=2e-5, what="gat fwd")
    close(dx, ref["gat_dx"], atol=2e-5, rel=1e-5, what="gat dx")
    for c in range(d["C"]):
        close(dwa[c], ref["gat_dwa"][c], atol=2e-5, rel=2e-5, what="gat dweight_a[%d]" % c)
    # rows without entries in any channel (padded rows, empty graphs, a single node without its self loop): sigmoid(0) per channel
    stored = np.zeros((d["T"], d["M"]), bool)
    for t, chans in enumerate(d["adjs"]):
        for idx, _v, _s in chans:
            stored[t, idx[:, 0]] = True
    pad = np.arange(d["M"])[None, :] >= d["sizes"][:, None]
    assert pad.any() and not stored[pad].any()
    empty = out[torch.as_tensor(~stored, device=out.device)]
    assert empty.numel() and float(empty.min()) == 0.5 * d["C"] == float(empty.max())
    # no atomics: a second forward and backward give the same bits
    again = _gat_run(d, adj)
    assert torch.equal(out, again[0]) and torch.equal(dx, again[1])
    assert all(torch.equal(a, b) for a, b in zip(dwa, again[2]))


def _maxpool_run(d, adj, x):
    from kgcn_amd import layers, ops
    tx = t32(x).requires_grad_(True)
    out = layers.GraphMaxPooling(d["C"])(tx, adj=adj) if d["M"] == d["K"] else ops.graph_maxpool(tx, adj)
    out.backward(t32(d["g"]))
    return out.detach(), tx.grad


@pytest.mark.parametrize("case", sorted(L.CASES))
def test_maxpool_against_the_oracle(case):
    """generic data against the fp64 oracle (default tolerance); grid data, where ties are real, against its fp32 form: the forward
    exactly, the gradient to 2e-6"""
    d = L.make_case(case)
    ref = d["ref"]
    row_pad = torch.as_tensor(np.arange(d["M"])[None, :] >= d["sizes"][:, None], device=dev())
    col_pad = torch.as_tensor(np.arange(d["K"])[None, :] >= d["col_sizes"][:, None], device=dev())
    for data, adjs, fwd, bwd, tol in ((d["x_pool"], d["adjs"], "mp_out", "mp_dx", None), (d["xg"], d["adjs_grid"], "mpg_out", "mpg_dx", (0, 2e-6))):
        adj = _adjacency(d, adjs)
        out, dx = _maxpool_run(d, adj, data)
        assert tuple(out.shape) == (d["T"], d["M"], d["D"]) and tuple(dx.shape) == (d["T"], d["K"], d["D"])
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all())
        if tol is None:
            close(out, ref[fwd], what="maxpool fwd (generic)")
            close(dx, ref[bwd], what="maxpool bwd (generic)")
        else:
            close(out, ref[fwd], atol=tol[0], what="maxpool fwd (grid)")
            close(dx, ref[bwd], atol=tol[1], what="maxpool bwd (grid)")
        assert bool(row_pad.any()) and not bool(out[row_pad].any()) and not bool(dx[col_pad].any())
        again = _maxpool_run(d, adj, data)
        assert torch.equal(out, again[0]) and torch.equal(dx, again[1])


def test_refusals_through_the_c_abi():
    """every refusal returns from validation: nothing is launched, the outputs keep their fill"""
    from kgcn_amd import BatchedCSR, _lib
    lib, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream()
    d = L.make_case("narrow")
    T, N, D = d["T"], d["M"], d["D"]
    mats = [a[0] for a in d["adjs"]]
    a = BatchedCSR.from_coo_list(mats, rows=N, cols=N, device=dev())
    at = a.transpose()
    other = BatchedCSR.from_coo_list([a[1] for a in d["adjs"]], rows=N, cols=N, device=dev()).transpose()
    assert other.nnz != a.nnz
    keep = [m[0][:, 0] < N - 1 for m in mats]               # the same graphs without their last row: [N - 1 x N]
    rect = BatchedCSR.from_coo_list([(m[0][k], m[1][k], [N - 1, N]) for m, k in zip(mats, keep)], rows=N - 1, cols=N, device=dev())
    x, g, wa = t32(d["x"]), t32(d["g"]), t32(d["weight_a"][0].reshape(-1))
    fill = 7.0
    out, dx, dw = (torch.full(s, fill, device=dev()) for s in ((T, N, D), (T, N, D), (2 * D,)))
    wsb = lib.kgcn_gat_workspace_bytes(T, N, D)
    ws = _lib.workspace(wsb, dev())
    mwsb = lib.kgcn_graph_maxpool_bwd_workspace_bytes(T, N, D)
    mws = _lib.workspace(mwsb, dev())
    assert wsb > 0 and mwsb == 2 * T * N * D * 4

    def gat_fwd(adj=a, beta=0.0, nbytes=wsb):
        return lib.kgcn_gat_fwd_f32(adj.desc(), ptr(x), D, ptr(wa), ptr(out), beta, ptr(ws), nbytes, stream)

    def gat_bwd(adj_t=at, beta=0.0, nbytes=wsb):
        return lib.kgcn_gat_bwd_f32(a.desc(), adj_t.desc(), ptr(x), D, ptr(wa), ptr(g), ptr(dx), beta, ptr(dw), ptr(ws), nbytes, stream)

    def mp_bwd(adj_t=at, beta=0.0, nbytes=mwsb):
        return lib.kgcn_graph_maxpool_bwd_f32(a.desc(), adj_t.desc(), ptr(x), ptr(g), D, ptr(dx), beta, ptr(mws), nbytes, stream)

    def mp_fwd(beta=0.0):
        return lib.kgcn_graph_maxpool_fwd_f32(a.desc(), ptr(x), D, ptr(out), beta, stream)

    refused = [
        (lambda: gat_fwd(adj=rect), b"square"),
        (lambda: gat_bwd(adj_t=rect.transpose()), b"transposed batch"),          # shape
        (lambda: gat_bwd(adj_t=other), b"transposed batch"),                     # nnz
        (lambda: mp_bwd(adj_t=rect.transpose()), b"transposed batch"),
        (lambda: mp_bwd(adj_t=other), b"transposed batch"),
        (lambda: gat_fwd(nbytes=wsb - 1), b"workspace"),
        (lambda: gat_bwd(nbytes=wsb - 1), b"workspace"),
        (lambda: mp_bwd(nbytes=mwsb - 1), b"workspace"),
    ]
    for beta in (0.5, 2.0, -1.0, float("nan")):
        refused += [(lambda f=f, beta=beta: f(beta=beta), b"beta") for f in (gat_fwd, gat_bwd, mp_bwd, mp_fwd)]
    for i, (call, word) in enumerate(refused):
        assert call() != 0 and word in lib.kgcn_last_error(), (i, word, lib.kgcn_last_error())
    with pytest.raises(_lib.KgcnHipError):
        _lib.check(gat_fwd(adj=rect), "kgcn_gat_fwd_f32")
    torch.cuda.synchronize()
    assert all(bool((t == fill).all()) for t in (out, dx, dw))
    # and the same arguments, unspoilt, are accepted
    assert gat_fwd() == 0 and gat_bwd() == 0 and mp_bwd() == 0 and mp_fwd() == 0
    torch.cuda.synchronize()
    assert not bool((dw == fill).any())
