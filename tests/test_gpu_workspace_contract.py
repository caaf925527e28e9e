"""The workspace contract of the C entry points that carve a caller's workspace (csrc/workspace.h; graphkern, hashkern, pairrank,
cvmetrics, linkpred, svm and labelprop), each called through _lib at the smallest shape that still uses every array of its layout:

  (a) one byte short of what the entry point needs: refused with `workspace <need - 1> < <need> bytes`, no output touched;
  (b) exactly that many bytes: the call succeeds;
  (c) the same number of bytes starting 8 bytes past a 256-byte boundary: every output has the bytes of (b).  Torch's own
      allocations are aligned, so no other test runs the path that rounds the caller's pointer up.
  In (b) and (c) the workspace lies inside a larger buffer of a known byte; no byte before it or past its `need` bytes changes.

`need` is what the entry point itself names when it is handed no bytes at all; it is the size its *_workspace_bytes query returns
(kgcn_pair_rank_table_i32 needs less than the query, which covers the select and the emit of the same ranking too).  No contract in
include/kgcn_hip.h asks for an aligned workspace, so (c) holds for all of them.  The *_copies_i32 entry points are the plain ones'
launchers with copies > 1 and are not repeated here."""
import ctypes
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -7


def up(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda")


def filled(shape, dtype):
    import torch
    return torch.full(shape, SENTINEL % 256 if dtype == torch.uint8 else SENTINEL, device="cuda", dtype=dtype)


def bytes_of(t):
    return t.cpu().numpy().reshape(-1).view(np.uint8)


def contract(entry, call, outputs, query=None, exact=True, prepare=None):
    """call(outs, ws, nbytes) -> rc with ws a uint8 tensor; outputs() -> fresh sentinel-filled outputs; prepare(ws, nbytes) fills a
    workspace with what an earlier call of the protocol leaves in it."""
    import torch
    from kgcn_amd import _lib
    empty = torch.empty((1,), device="cuda", dtype=torch.uint8)
    assert call(outputs(), empty, 0) == 1
    m = re.search(r"^%s: workspace 0 < (\d+) bytes$" % entry, _lib.lib.kgcn_last_error().decode())
    assert m, _lib.lib.kgcn_last_error()
    need = int(m.group(1))
    if query is not None:
        assert need == query if exact else 0 < need <= query, (need, query)
    big = torch.empty((need + 512,), device="cuda", dtype=torch.uint8)
    a0 = (-big.data_ptr()) % 256
    aligned, skewed = big[a0:a0 + need], big[a0 + 8:a0 + 8 + need]
    assert aligned.data_ptr() % 256 == 0 and skewed.data_ptr() % 256 == 8
    # (a)
    outs = outputs()
    before = [bytes_of(t) for t in outs]
    assert call(outs, aligned, need - 1) == 1
    assert _lib.lib.kgcn_last_error().decode() == "%s: workspace %d < %d bytes" % (entry, need - 1, need)
    torch.cuda.synchronize()
    for t, b in zip(outs, before):
        np.testing.assert_array_equal(bytes_of(t), b)
    # (b), (c)
    got = []
    for ws in (aligned, skewed):
        big.fill_(0xA5)
        if prepare is not None:
            prepare(ws, need)
        outs = outputs()
        assert call(outs, ws, need) == 0, _lib.lib.kgcn_last_error()
        torch.cuda.synchronize()
        got.append([bytes_of(t) for t in outs])
        first = ws.data_ptr() - big.data_ptr()                        # nothing outside the `need` bytes handed in is written
        assert bool((big[:first] == 0xA5).all()) and bool((big[first + need:] == 0xA5).all())
    for b, c in zip(*got):
        np.testing.assert_array_equal(b, c)
    return need


def two_graphs():
    """2 graphs x 3 rows: a path of three nodes, and an edge of two nodes with one padded row"""
    from kgcn_amd.batched_csr import BatchedCSR
    g, r, c = np.array([0, 0, 0, 0, 1, 1]), np.array([0, 1, 1, 2, 0, 1]), np.array([1, 0, 2, 1, 1, 0])
    csr = BatchedCSR.from_arrays(g, r, c, np.ones(6, np.float32), 2, 3, 3)
    return csr, up(np.array([3, 2], np.int32)), up(np.array([0, 0, 0, 0, 0, -1], np.int32))


def test_wl_rank():
    import torch
    from kgcn_amd import _lib, ops
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    csr, nn, colours = two_graphs()
    sorted_nbr, khi, klo = ops.wl_refine(csr, nn, colours)
    contract("kgcn_wl_rank_i32",
             lambda o, ws, nb: L.kgcn_wl_rank_i32(ctypes.byref(csr.desc()), ptr(nn), ptr(colours), ptr(sorted_nbr), ptr(khi), ptr(klo),
                                                  ptr(o[0]), ptr(o[1]), ptr(ws), nb, stream()),
             lambda: [filled((6,), torch.int32), filled((2,), torch.int64)], L.kgcn_wl_rank_workspace_bytes(6))
    new, info = ops.wl_rank(csr, nn, colours, sorted_nbr, khi, klo)
    new = new.tolist()
    assert sorted(new[:2]) == [0, 1] and new[2:] == [new[0], new[0], new[0], -1] and info.tolist() == [2, 0]


def test_rank_pairs():
    import torch
    from kgcn_amd import _lib
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    hi, lo = up(np.array([3, 1, 3, 2, 1], np.int64)), up(np.array([0, 5, 0, 9, 7], np.int64))
    mark = up(np.array([0, 0, 0, -1, 0], np.int32))                  # one row that does not exist, rows 0 and 2 equal
    last = []

    def call(o, ws, nb):
        last[:] = o
        return L.kgcn_rank_pairs_i64(ptr(hi), ptr(lo), ptr(mark), 5, ptr(o[0]), ptr(o[1]), ptr(ws), nb, stream())

    contract("kgcn_rank_pairs_i64", call, lambda: [filled((5,), torch.int32), filled((2,), torch.int64)],
             L.kgcn_rank_pairs_workspace_bytes(5))
    assert last[0].tolist() == [2, 0, 2, -1, 1] and last[1].tolist() == [3, 0]


def test_runs_in_count_mode():
    import torch
    from kgcn_amd import _lib
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    csr, nn, colours = two_graphs()
    labels = up(np.zeros(6, np.int32))
    need = L.kgcn_graph_runs_workspace_bytes(2)
    out = lambda: [filled((3,), torch.int64)]
    contract("kgcn_wl_runs_i32",
             lambda o, ws, nb: L.kgcn_wl_runs_i32(ptr(colours), ptr(nn), 2, 3, 0, ptr(o[0]), None, None, None, 0, ptr(ws), nb, stream()),
             out, need)
    contract("kgcn_sp_features_i32",
             lambda o, ws, nb: L.kgcn_sp_features_i32(ctypes.byref(csr.desc()), ptr(nn), ptr(labels), 1, ptr(o[0]), None, None, None, 0,
                                                      ptr(ws), nb, stream()),
             out, need)


def test_gram_plan_and_dense():
    import torch
    from kgcn_amd import _lib
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    col, graph, count = up(np.array([9, 9, 4, 5], np.int64)), up(np.array([0, 1, 0, 1], np.int32)), up(np.array([1, 2, 3, 4], np.int32))
    need = L.kgcn_graph_gram_workspace_bytes(4, 2, 16)
    last = []

    def plan(o, ws, nb):
        last[:] = o
        return L.kgcn_gram_plan_i64(ptr(col), ptr(graph), ptr(count), 4, 2, 16, ptr(o[0]), ptr(ws), nb, stream())

    def dense(o, ws, nb):
        last[:] = o
        return L.kgcn_gram_dense_f64(ptr(graph), ptr(count), 4, 2, 1, 16, ptr(o[0]), ptr(ws), nb, stream())

    contract("kgcn_gram_plan_i64", plan, lambda: [filled((3,), torch.int64)], need)
    assert last[0].tolist() == [3, 2, 1]
    contract("kgcn_gram_dense_f64", dense, lambda: [filled((2, 2), torch.float64)], need,
             prepare=lambda ws, nb: plan([filled((3,), torch.int64)], ws, nb))
    assert last[0].tolist() == [[1 + 9, 2], [2, 4 + 16]]


def test_attr_scale():
    import torch
    from kgcn_amd import _lib
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    x = up(np.array([[1.0, 2.0], [3.0, 2.0], [8.0, -1.0]]))
    contract("kgcn_attr_scale_f64",
             lambda o, ws, nb: L.kgcn_attr_scale_f64(ptr(x), 3, 2, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(ws), nb, stream()),
             lambda: [filled((3, 2), torch.float64), filled((2,), torch.float64), filled((2,), torch.float64)],
             L.kgcn_attr_scale_workspace_bytes(3, 2))


def test_binary_metrics():
    import torch
    from kgcn_amd import _lib
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    score = up(np.array([[0.9, 0.2], [0.4, 0.7], [0.6, 0.7]], np.float32))
    label = up(np.array([[1, 0], [0, 1], [1, 1]], np.float32))
    contract("kgcn_binary_metrics_f32",
             lambda o, ws, nb: L.kgcn_binary_metrics_f32(ptr(score), 2, ptr(label), None, 3, 2, 0.5, ptr(o[0]), ptr(o[1]), ptr(ws), nb,
                                                         stream()),
             lambda: [filled((2, 8), torch.int64), filled((2,), torch.float64)], L.kgcn_binary_metrics_workspace_bytes(3, 2))


def test_pair_rank():
    import torch
    from kgcn_amd import _lib
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    h = up(np.array([[1.0], [2.0], [-1.0]], np.float32))              # 3 nodes, dim 1: scores 2, -1, -2
    last = []

    def select(o, ws, nb):
        last[:] = o
        return L.kgcn_pair_rank_select_f32(ptr(h), 3, 1, None, 0, ptr(o[0]), ptr(ws), nb, stream())

    contract("kgcn_pair_rank_select_f32", select, lambda: [filled((3,), torch.int64)], L.kgcn_pair_rank_workspace_bytes(3, 1, 0, 0))
    counts = last[0]
    capacity = int(counts[1]) + int(counts[2])
    assert capacity == 3

    def emit(o, ws, nb):
        last[:] = o
        return L.kgcn_pair_rank_emit_f32(ptr(h), 3, 1, None, 0, ptr(counts), capacity, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(ws), nb,
                                         stream())

    contract("kgcn_pair_rank_emit_f32", emit, lambda: [filled((3,), torch.float32), filled((3,), torch.int32), filled((3,), torch.int32)],
             L.kgcn_pair_rank_workspace_bytes(3, 1, capacity, 0))
    score, row, col = last
    assert (score.tolist(), row.tolist(), col.tolist()) == ([2.0, -1.0, -2.0], [0, 0, 1], [1, 2, 2])
    target, test = up(np.array([1, (1 << 16) | 2], np.int32)), up(np.array([(1 << 16) | 2], np.int32))
    top = (ctypes.c_int64 * 1)(2)
    contract("kgcn_pair_rank_table_i32",
             lambda o, ws, nb: L.kgcn_pair_rank_table_i32(ptr(score), ptr(row), ptr(col), 3, ptr(target), 2, ptr(test), 1, top, 1,
                                                          ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), ptr(o[4]), ptr(o[5]), ptr(ws), nb,
                                                          stream()),
             lambda: [filled((3,), torch.uint8) for _ in range(3)] + [filled((3,), torch.int64), filled((1,), torch.int64),
                                                                     filled((1,), torch.int64)],
             L.kgcn_pair_rank_workspace_bytes(2, 1, 0, 3), exact=False)


def test_svm_smo():
    import torch
    from kgcn_amd import _lib, ops
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    x = np.array([[0.0, 1.0], [1.0, 2.0], [3.0, 0.5], [4.0, 0.0]])
    K = up(x @ x.T + np.eye(4))
    sets = ops.SvmSets([[0, 1, 2, 3]], [[1, 1, -1, -1]], graphs=4)   # one problem of 4 rows
    prob_set, prob_C, tol = up(np.zeros(1, np.int32)), up(np.ones(1)), ctypes.c_double(1e-3)
    last = []

    def call(o, ws, nb):
        last[:] = o
        return L.kgcn_svm_smo_f64(ptr(K), 4, *sets.args(), ptr(prob_set), ptr(prob_C), 1, ctypes.byref(tol), 0, ops.SVM_DEFAULT_SLICE, 1,
                                  ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(o[3]), ptr(ws), nb, stream())

    contract("kgcn_svm_smo_f64", call,
             lambda: [filled((1, 4), torch.float64), filled((1,), torch.float64), filled((1,), torch.int64), filled((1,), torch.int32)],
             L.kgcn_svm_workspace_bytes(1, 4))
    assert last[3].tolist() == [ops.SVM_CONVERGED]


def test_label_propagation():
    import torch
    from kgcn_amd import _lib, ops
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    x = up(np.array([[0.0, 0.0], [1.0, 1.0], [0.2, 0.1], [0.9, 1.2], [0.5, 0.5]]))   # 5 points, 1 task, 2 columns
    gamma, alpha, tol = ctypes.c_double(0.5), ctypes.c_double(0.2), ctypes.c_double(1e-3)
    W = ops.rbf_affinity(x, gamma.value)
    s, _ = ops.lp_degrees(W)
    labels, task_col = up(np.array([[0], [1], [-1], [-1], [-1]], np.int32)), up(np.array([0, 2], np.int32))
    need = L.kgcn_lp_workspace_bytes(5, 1, 2)
    tail = lambda o, ws, nb: (5, ptr(labels), ptr(task_col), 1, 2, _lib.K["KGCN_LP_PROPAGATION"], ctypes.byref(alpha), ctypes.byref(tol),
                              1000, 0, 3, ptr(o[0]), ptr(o[1]), ptr(ws), nb, stream())
    stored = lambda o, ws, nb: L.kgcn_lp_propagate_f64(ptr(W), ptr(s), *tail(o, ws, nb))
    free = lambda o, ws, nb: L.kgcn_lp_propagate_free_f64(ptr(x), 2, ctypes.byref(gamma), ptr(o[2]), ptr(s), *tail(o, ws, nb))
    meta = lambda: [filled((1,), torch.int32), filled((1,), torch.int32)]
    contract("kgcn_lp_propagate_f64", stored, meta, need)
    contract("kgcn_lp_propagate_free_f64", free, lambda: meta() + [filled((5,), torch.float64)], need)
    last = []

    def finish(o, ws, nb):
        last[:] = o
        return L.kgcn_lp_finish_f64(5, ptr(task_col), 1, 2, 3, ptr(o[0]), ptr(ws), nb, stream())

    contract("kgcn_lp_finish_f64", finish, lambda: [filled((5, 2), torch.float64)], need, prepare=lambda ws, nb: stored(meta(), ws, nb))
    dist = last[0].cpu().numpy()
    assert dist[:2].tolist() == [[1.0, 0.0], [0.0, 1.0]] and np.all(dist > -1.0) and np.all(np.abs(dist.sum(1) - 1.0) < 1e-12)


def test_linkpred_bwd():
    import torch
    from kgcn_amd import _lib
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    mode = _lib.K["KGCN_LP_DISTMULT"]                                 # the mode that uses every array: the d w partials too
    h = up(np.array([[1.0, 0.5], [0.25, -1.0], [2.0, 1.0], [-0.5, 0.75]], np.float32))
    w = up(np.array([[1.0, -2.0]], np.float32))
    labels, negatives = up(np.array([[0, 0, 1, 0, 0, 2]], np.int32)), up(np.array([0, 1, 2, 3], np.int32))
    rows, s1, s2, sums = filled((1, 6), torch.int32), filled((1,), torch.float32), filled((1,), torch.float32), filled((5,), torch.float32)
    assert L.kgcn_linkpred_fwd_f32(ptr(h), 4, 2, ptr(w), 1, mode, ptr(labels), None, 1, 1, ptr(negatives), 4, 7, None, ptr(rows), ptr(s1),
                                   ptr(s2), ptr(sums), stream()) == 0
    g_opt = up(np.ones(1, np.float32))
    contract("kgcn_linkpred_bwd_f32",
             lambda o, ws, nb: L.kgcn_linkpred_bwd_f32(ptr(h), 4, 2, ptr(w), 1, mode, ptr(rows), ptr(s1), ptr(s2), ptr(sums), 1, ptr(g_opt),
                                                       None, ptr(o[0]), ptr(o[1]), ptr(ws), nb, stream()),
             lambda: [filled((4, 2), torch.float32), filled((1, 2), torch.float32)], L.kgcn_linkpred_workspace_bytes(4, 2, 1, mode, 1))
