"""The fused GraphConv kernels (kgcn_amd/csrc/fused.hip) on directed, dense and long-row graphs (tests/fused_cases.py), every result
against the fp64 reference of the DENSE adjacency -- never against another kernel's output:
  * through the layer route (BatchedCSR.from_coo_list / from_arrays on the unsorted triples, ops.graphconv_fused), with and without
    a gradient for x (the first layer of every model: the generic backward at the FULL shape),
  * through the C entry points with the row-padded descriptor and, where the library accepts it, the compact one.
What is reached: the FULL forward in LAY_PAD4 / LAY_UNIT / LAY_VALS on A != A^T, the planes backward (T = 5), the pairs backward in
each layout (T = 2049: one pair owns three graphs) and its streaming form (`directed` at the first T of bwd_streams), the generic
backward at the FULL shape from 224 row-padded entries on and with no dX, and the "> 256 entries" loops of land_csr (complete,
row252: the row-padded forward), land_csr_c (k12: the compact forward) and land_csr_p (pack2, pack4).  The route witnesses make a case
fail loudly, rather than silently move off its edge, when the LDS budgeting changes.
Tolerances: the forms of test_graphconv_fused; fused_cases.COMPONENTWISE where float32 itself does not keep a quarter of them."""
import ctypes

import numpy as np
import pytest
import torch

import conftest
import fused_cases as F
from test_gpu_parity import close, dev, t32

pytestmark = pytest.mark.gpu

COMPACT = 0x104
LABEL = {"fwd": "fwd", "dx": "dX", "dw": "dW", "db": "dbias"}
RUNS = [(name, T, with_dx) for name, T in F.gpu_runs() for with_dx in (True, False)]
C_RUNS = [(name, T) for name in F.FULL_CASES for T in (5, 2049)]


def check(name, T, what, got, ref, route):
    """close() in the written form, or the componentwise bound of fused_cases.COMPONENTWISE; label: case, route, quantity"""
    label = "%s %s %s" % (name, route, LABEL[what])
    r = np.asarray(getattr(ref, what))
    got = got.detach().cpu().numpy().reshape(r.shape)
    comp = F.COMPONENTWISE.get((name, T, what))
    if comp is None:
        return close(got, r, atol=F.ATOL, rel=F.REL[what], what=label)
    bound = 4.0 * comp * F.EPS * np.asarray(ref.s_dw if what == "dw" else ref.s_db).reshape(r.shape)
    err = np.abs(got.astype(np.float64) - r)
    i = np.unravel_index(np.argmax(err / bound), err.shape)
    conftest.record_accuracy(label + " (componentwise)", float(err[i]), float(bound[i]), float(np.abs(r).max()), float(bound[i]))
    assert err[i] <= bound[i], "%s: err %.3e > %.1f * 2^-24 * S = %.3e at %s" % (label, err[i], 4.0 * comp, bound[i], i)


def up(a):
    """to the device; the cases' arrays are read-only and shared between tests: upload a copy"""
    return t32(np.array(a))


def container(case, coo):
    from kgcn_amd import BatchedCSR
    if coo:
        return BatchedCSR.from_coo_list(F.coo_list(case), rows=case.N, cols=case.N, device=dev())
    return BatchedCSR.from_arrays(case.graph, case.row, case.col, case.val, case.T, case.N, case.N, device=dev())


def expect_pairs(case, with_dx):
    """bwd_pairs_route restated: a gradient for x, the planes slice fits (<= 220 row-padded entries), >= 2,048 graphs"""
    return bool(with_dx and case.N == 32 and case.padded_t.max() <= 220 and case.T >= 2048)


@pytest.mark.parametrize("name,T,with_dx", RUNS)
def test_layer_route(name, T, with_dx):
    from kgcn_amd import ops
    from kgcn_amd._lib import lib
    case, op, ref = F.build(name, T), F.operands(name, T), F.reference(name, T)
    N, din, dout = case.N, case.din, case.dout
    csr = container(case, coo=with_dx)
    assert ops.graphconv_fused_supported(csr, din, dout)
    # ---- where the case is: sizes, layouts, kernels ----
    p4, p4t = csr.padded4(), csr.transpose().padded4()
    assert (p4.max_nnz, p4t.max_nnz) == (int(case.padded.max()), int(case.padded_t.max()))
    pairs = expect_pairs(case, with_dx)
    assert bool(lib.kgcn_graphconv_fused_reads_compact(1, T, N, din, dout, p4t.max_nnz, int(with_dx))) == pairs
    if N == 32:
        c4, c4t = p4.compact4(), p4t.compact4()
        assert (c4 is not None, c4t is not None) == (case.compact_ok, case.compact_ok_t)
        assert c4 is None or c4.unit_values == (name == "directed_unit")
        assert ops._fused_adjacency(csr, False, T, din, dout, False).row_pad == (COMPACT if case.compact_ok else 4)
        assert ops._fused_adjacency(csr.transpose(), True, T, din, dout, with_dx).row_pad == \
            (COMPACT if pairs and case.compact_ok_t else 4)
    else:
        assert ops._fused_adjacency(csr, False, T, din, dout, False).row_pad == 4
    if T == F.stream_T():
        assert T * 32 * 64 * 4 * 3 > (256 << 20) and pairs == with_dx        # the streaming instantiation of the pairs kernel
    # ---- the values ----
    route = "layer" if with_dx else "layer, no dX"
    tx, tw, tb = up(op.x).requires_grad_(with_dx), up(op.w).requires_grad_(True), up(op.b).requires_grad_(True)
    out = ops.graphconv_fused(tx, tw, tb, csr)
    check(name, T, "fwd", out, ref, route)
    out.backward(up(op.g))
    if with_dx:
        check(name, T, "dx", tx.grad, ref, route)
    else:
        assert tx.grad is None
    check(name, T, "dw", tw.grad, ref, route)
    check(name, T, "db", tb.grad, ref, route)


def c_fwd(desc, x, w, b, D):
    from kgcn_amd._lib import lib, ptr, current_stream, check as ok
    out = torch.full_like(x, float("nan"))
    ok(lib.kgcn_graphconv_fwd_f32(desc, ptr(x), ptr(w), ptr(b), D, D, ptr(out), current_stream()), "kgcn_graphconv_fwd_f32")
    return out


def c_bwd(desc, x, w, g, D, rc_only=False):
    from kgcn_amd._lib import lib, ptr, current_stream, check as ok
    wsb = lib.kgcn_graphconv_bwd_workspace_bytes(x.shape[0], D, D)
    wsp = torch.empty(max(1, wsb // 4), device=dev())
    dx = torch.full_like(x, float("nan"))
    dw, db = torch.empty((D, D), device=dev()), torch.empty(D, device=dev())
    rc = lib.kgcn_graphconv_bwd_f32(desc, ptr(x), ptr(w), ptr(g), D, D, ptr(dx), ptr(dw), ptr(db), ptr(wsp), wsb, current_stream())
    if rc_only:
        return rc
    ok(rc, "kgcn_graphconv_bwd_f32")
    return dx, dw, db


def as_compact(p4):
    """the row-padded descriptor relabelled compact: for launches the library refuses on its host side, before it picks a kernel
    (nothing reads the arrays)"""
    from kgcn_amd import _lib
    d = _lib.CsrBatch()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(p4.desc()), ctypes.sizeof(_lib.CsrBatch))
    d.row_pad = COMPACT
    return d


@pytest.mark.parametrize("name,T", C_RUNS)
def test_c_entry_points(name, T):
    from kgcn_amd._lib import lib
    case, op, ref = F.build(name, T), F.operands(name, T), F.reference(name, T)
    D = 64
    csr = container(case, coo=False)
    p4, p4t = csr.padded4(), csr.transpose().padded4()
    c4, c4t = p4.compact4(), p4t.compact4()
    assert (c4 is not None, c4t is not None) == (case.compact_ok, case.compact_ok_t)
    x, w, b, g = up(op.x), up(op.w), up(op.b).reshape(-1), up(op.g)
    check(name, T, "fwd", c_fwd(p4.desc(), x, w, b, D), ref, "C row-padded")
    for what, got in zip(("dx", "dw", "db"), c_bwd(p4t.desc(), x, w, g, D)):
        check(name, T, what, got, ref, "C row-padded")
    if c4 is not None:
        assert c4.unit_values == (name == "directed_unit")
        check(name, T, "fwd", c_fwd(c4.desc(), x, w, b, D), ref, "C compact")
    pairs = expect_pairs(case, True)
    assert bool(lib.kgcn_graphconv_fused_reads_compact(1, T, 32, D, D, p4t.max_nnz, 1)) == pairs
    if pairs and c4t is not None:
        for what, got in zip(("dx", "dw", "db"), c_bwd(c4t.desc(), x, w, g, D)):
            check(name, T, what, got, ref, "C compact")
    elif not pairs:                                       # the planes and the generic backward read row_pad = 4 only
        assert c_bwd(c4t.desc() if c4t is not None else as_compact(p4t), x, w, g, D, rc_only=True) != 0
        assert b"compact" in lib.kgcn_last_error()


def test_route_witnesses():
    """edge220 is the last size on the planes / pairs kernels, edge224 the first on the generic one; where the compact layout
    cannot hold a batch (row64) the pairs kernel reads the row-padded copy through the layer"""
    from kgcn_amd import ops
    from kgcn_amd._lib import lib
    for name, reads in (("edge220", 1), ("edge224", 0)):
        case = F.build(name, 2049)
        p4t = container(case, coo=False).transpose().padded4()
        assert p4t.max_nnz == int(name[4:])
        assert lib.kgcn_graphconv_fused_reads_compact(1, 2049, 32, 64, 64, p4t.max_nnz, 1) == reads
        assert lib.kgcn_graphconv_fused_reads_compact(1, 2049, 32, 64, 64, p4t.max_nnz, 0) == 0      # no dX: the generic kernel
    expect = {"directed": True, "directed_unit": True, "edge220": True, "edge224": True, "k12": True, "complete": False,
              "row64": False, "row252": False}
    for name, has in expect.items():
        c4 = container(F.build(name, 5), coo=False).padded4().compact4()
        assert (c4 is not None) == has, name
        assert c4 is None or c4.unit_values == (name == "directed_unit"), name
    case = F.build("row64", 2049)
    csr = container(case, coo=True)
    assert lib.kgcn_graphconv_fused_reads_compact(1, 2049, 32, 64, 64, csr.transpose().padded4().max_nnz, 1) == 1
    assert ops._fused_adjacency(csr.transpose(), True, 2049, 64, 64, True).row_pad == 4
    assert ops._fused_adjacency(csr, False, 2049, 64, 64, False).row_pad == 4


@pytest.mark.parametrize("build", ["host", "device"])
def test_row_of_256_padded_entries_is_refused(build):
    """One row of 256 entries: the 8-bit length of the slot word cannot hold it.  It never reaches a fused kernel truncated: building
    the row-padded copy raises, from the numpy packer and from kgcn_csr_pad4's count (stats[2]) alike -- and so does the layer."""
    from kgcn_amd import BatchedCSR, layers, ops
    case = F.build("row256", 5)
    if build == "host":
        csr = BatchedCSR.from_arrays(case.graph, case.row, case.col, case.val, 5, 32, 32, device=dev())
    else:
        i32 = lambda a: torch.as_tensor(np.asarray(a, np.int32), device=dev())
        csr = BatchedCSR.from_device_coo(i32(case.graph), i32(case.row), i32(case.col), up(case.val), 5, 32, 32)
    with pytest.raises(ValueError, match="too dense for the packed slot table"):
        csr.padded4()
    with pytest.raises(ValueError, match="too dense for the packed slot table"):
        csr.transpose().transpose().padded4()             # nothing half-built was cached
    layer = layers.GraphConv(64, 1)
    with pytest.raises(ValueError, match="too dense for the packed slot table"):
        layer(up(F.operands("row256", 5).x), adj=csr)
    # one copy fewer (252 entries) is the longest row the slot word holds: that batch builds
    ok = F.build("row252", 5)
    assert BatchedCSR.from_arrays(ok.graph, ok.row, ok.col, ok.val, 5, 32, 32, device=dev()).padded4().max_nnz == 376
    assert ops.graphconv_fused_supported(csr, 64, 64)     # the shape test alone does not see the row: the packer refuses
