"""The compact row-padded adjacency (KGCN_ROW_PAD_COMPACT, BatchedCSR.compact4()) read by the FULL-shape fused GraphConv
kernels: the device packer against a numpy restatement of the layout, and the forward output / backward dX, dW, dbias
through the compact copy bit-equal to the same kernels fed padded4() (same entries, same order of the sums)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, D = 32, 64


def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def make_batch(T, normalize, seed=0):
    """T graphs of 32 nodes: duplicate entries, empty rows, empty graphs (every 7th), rows longer than 8 entries (row 3 of
    every 5th graph: 20 entries, repeated columns among them); unit values or positive weights.  At most ~210 row-padded
    entries per graph, within the FULL backward's LDS slice (the pairs kernel takes the batch from 2,048 graphs on)."""
    from kgcn_amd import BatchedCSR
    rng = np.random.default_rng(seed + T)
    counts = rng.integers(30, 90, size=T)
    counts[::7] = 0
    g = np.repeat(np.arange(T), counts)
    r = rng.integers(0, N, size=g.shape[0])
    c = rng.integers(0, N, size=g.shape[0])
    lg = np.arange(1, T, 5)
    g = np.concatenate([g, np.repeat(lg, 20)])
    r = np.concatenate([r, np.full(lg.shape[0] * 20, 3)])
    c = np.concatenate([c, np.tile(np.arange(20) % 10, lg.shape[0])])
    order = np.argsort(g, kind="stable")
    g, r, c = g[order], r[order], c[order]
    v = rng.uniform(0.05, 1.0, size=g.shape[0]).astype(np.float32) if normalize else np.ones(g.shape[0], np.float32)
    return BatchedCSR.from_arrays(g, r, c, v, T, N, N, device=dev())


def features(T, seed):
    gen = torch.Generator(device=dev())
    gen.manual_seed(seed)
    a = torch.randn((T, N, D), device=dev(), generator=gen)
    a[0, 1, 2] = float("inf")
    a[min(1, T - 1), 5, 7] = float("nan")
    a[T - 1, 0, 0] = float("-inf")
    return a


def same_bits(a, b):
    """equal bit patterns everywhere, NaN where the other is NaN"""
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    return torch.equal(a.masked_fill(na, 0).view(torch.int32), b.masked_fill(nb, 0).view(torch.int32))


def fwd(desc, x, w, b):
    from kgcn_amd._lib import lib, ptr, current_stream, check
    out = torch.full_like(x, float("nan"))
    check(lib.kgcn_graphconv_fwd_f32(desc, ptr(x), ptr(w), ptr(b), D, D, ptr(out), current_stream()),
          "kgcn_graphconv_fwd_f32")
    return out


def bwd(desc, x, w, g, rc_only=False):
    from kgcn_amd._lib import lib, ptr, current_stream, check
    T = x.shape[0]
    wsb = lib.kgcn_graphconv_bwd_workspace_bytes(T, D, D)
    wsp = torch.empty(max(1, wsb // 4), device=dev())
    dx = torch.full_like(x, float("nan"))
    dw = torch.empty((D, D), device=dev())
    db = torch.empty(D, device=dev())
    rc = lib.kgcn_graphconv_bwd_f32(desc, ptr(x), ptr(w), ptr(g), D, D, ptr(dx), ptr(dw), ptr(db), ptr(wsp), wsb,
                                    current_stream())
    if rc_only:
        return rc
    check(rc, "kgcn_graphconv_bwd_f32")
    return dx, dw, db


def weights(seed):
    rng = np.random.default_rng(seed)
    w = torch.as_tensor(rng.uniform(-0.3, 0.3, size=(D, D)).astype(np.float32), device=dev())
    b = torch.as_tensor(rng.uniform(-0.1, 0.1, size=D).astype(np.float32), device=dev())
    return w, b


def restate_compact(p4):
    """numpy restatement of the compact layout from the row-padded container: column words, value stream, 16-bit slots"""
    cv = p4.cv.cpu().numpy()
    cols = cv[:, 0].astype(np.uint32)
    words = (cols[0::4] | (cols[1::4] << 8) | (cols[2::4] << 16) | (cols[3::4] << 24)).astype(np.uint32)
    vals = cv[:, 1].copy()
    real = cols != 32
    unit = bool(np.all(vals[real] == np.float32(1.0).view(np.int32)))
    s = p4.slots.cpu().numpy().view(np.uint32)
    off, ln, row = s & 0xFFFF, (s >> 16) & 0xFF, s >> 24
    slots16 = ((off >> 2) | ((ln >> 2) << 7) | (row << 11)).astype(np.uint16)
    return words, vals, unit, slots16


@pytest.mark.parametrize("normalize", [False, True])
def test_packer_matches_numpy_restatement(normalize):
    from kgcn_amd._lib import lib
    csr = make_batch(3000, normalize)
    for p4 in (csr.padded4(), csr.transpose().padded4()):
        c4 = p4.compact4()
        assert c4 is not None
        words, vals, unit, slots16 = restate_compact(p4)
        assert c4.unit_values == unit == (not normalize)
        got = c4.cv.cpu().numpy()
        assert np.array_equal(got[:words.shape[0]].view(np.uint32), words)
        if not unit:
            off = int(lib.kgcn_compact_values_offset(p4.nnz))
            assert np.array_equal(got[off:off + p4.nnz], vals)
        assert np.array_equal(c4.slots.cpu().numpy().view(np.uint16), slots16)
        d = c4.desc()
        assert (d.row_pad, d.reserved_) == (0x104, 1 if unit else 0)
        assert p4.compact4() is c4                                   # cached on the row-padded container


@pytest.mark.parametrize("T,normalize", [(T, nz) for T in (5, 2047, 2048, 2049, 5000) for nz in (False, True)] +
                         [(100000, False)])
def test_compact_bit_equal_to_padded(T, normalize):
    from kgcn_amd._lib import lib
    csr = make_batch(T, normalize)
    x, g = features(T, 1), features(T, 2)
    w, b = weights(3)
    p4, p4t = csr.padded4(), csr.transpose().padded4()
    c4, c4t = p4.compact4(), p4t.compact4()
    assert c4.unit_values == c4t.unit_values == (not normalize)
    assert same_bits(fwd(c4.desc(), x, w, b), fwd(p4.desc(), x, w, b)), "forward output"
    pairs = lib.kgcn_graphconv_fused_reads_compact(1, T, N, D, D, p4t.max_nnz, 1)
    assert pairs == (T >= 2048)
    if pairs:
        for got, ref, name in zip(bwd(c4t.desc(), x, w, g), bwd(p4t.desc(), x, w, g), ("dX", "dW", "dbias")):
            assert same_bits(got, ref), name
    else:                                                             # the planes kernel reads row_pad = 4 only
        assert bwd(c4t.desc(), x, w, g, rc_only=True) != 0
        assert b"compact" in lib.kgcn_last_error()


def test_pairs_backward_compact_repeats_bit_for_bit():
    csr = make_batch(5000, True)
    x, g = features(5000, 4), features(5000, 5)
    w, _ = weights(6)
    c4t = csr.transpose().padded4().compact4()
    first = bwd(c4t.desc(), x, w, g)
    for rep in range(300):
        again = bwd(c4t.desc(), x, w, g)
        for a, b, name in zip(first, again, ("dX", "dW", "dbias")):
            assert same_bits(a, b), "launch %d: %s differs from the first launch" % (rep, name)


def test_layer_routes_compact_and_matches_padded():
    """ops.graphconv_fused hands the compact copy to the FULL forward and the pairs backward, the row-padded one to the
    planes backward and to generic shapes; every result equals the row-padded launch's bits."""
    from kgcn_amd import ops
    for T in (2047, 2048):
        csr = make_batch(T, False, seed=7)
        assert ops._fused_adjacency(csr, False, T, D, D, False).row_pad == 0x104
        assert ops._fused_adjacency(csr.transpose(), True, T, D, D, True).row_pad == (0x104 if T >= 2048 else 4)
        assert ops._fused_adjacency(csr.transpose(), True, T, D, D, False).row_pad == 4      # no dX: generic kernel
        assert ops._fused_adjacency(csr, False, T, 32, D, False).row_pad == 4                # generic shape
        x, g = features(T, 8), features(T, 9)
        w, b = weights(10)
        xr = x.clone().requires_grad_(True)
        wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        out = ops.graphconv_fused(xr, wr, br, csr)
        out.backward(g)
        assert same_bits(out.detach(), fwd(csr.padded4().desc(), x, w, b))
        dx, dw, db = bwd(csr.transpose().padded4().desc(), x, w, g)
        assert same_bits(xr.grad, dx) and same_bits(wr.grad, dw) and same_bits(br.grad, db)


def test_generic_kernels_refuse_compact():
    from kgcn_amd._lib import lib, ptr, current_stream
    csr = make_batch(64, False)
    c4 = csr.padded4().compact4()
    x = torch.zeros((64, N, 32), device=dev())
    w = torch.zeros((32, D), device=dev())
    out = torch.empty((64, N, D), device=dev())
    assert lib.kgcn_graphconv_fwd_f32(c4.desc(), ptr(x), ptr(w), None, 32, D, ptr(out), current_stream()) != 0
    assert b"compact" in lib.kgcn_last_error()
    o2 = torch.empty((64 * N, D), device=dev())
    assert lib.kgcn_bspmm_f32(c4.desc(), ptr(o2), D, N * D, D, ptr(o2), D, N * D, 0.0, current_stream()) != 0
    assert b"row_pad" in lib.kgcn_last_error()
