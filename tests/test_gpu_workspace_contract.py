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
launchers with copies > 1 and are not repeated here.

The multi-array layouts of the training step's ops (bn, gat, max-pooling, seq, conv1d, cpi-ig, vae, dense, fused GraphConv, stack)
follow in the second half.  They are packed (carved at 4 bytes) and use the caller's pointer as it is, so (c) is not run for them: a
skewed pointer would be a misaligned access.  Where the layout declares a base alignment above 4 bytes (batch normalisation's
64-bit count, the 64-bit block sums of kgcn_ragged_plan), a base 4 bytes off is refused with `workspace not <n>-byte aligned` and no output is touched.  kgcn_graphconv_bwd_f32
and kgcn_gcn_stack_bwd_f32 need one partial per workgroup they launch, at most what their queries (sized for a full grid) return."""
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


def contract(entry, call, outputs, query=None, exact=True, prepare=None, packed_align=None):
    """call(outs, ws, nbytes) -> rc with ws a uint8 tensor; outputs() -> fresh sentinel-filled outputs; prepare(ws, nbytes) fills a
    workspace with what an earlier call of the protocol leaves in it.  packed_align: the entry point does not round its base (the
    packed layouts) and its layout declares this base alignment: (c) is not run; above 4, a base 4 bytes past the aligned one is
    refused by name with no output touched."""
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

    def refused(ws, nbytes, message):
        outs = outputs()
        before = [bytes_of(t) for t in outs]
        assert call(outs, ws, nbytes) == 1
        assert _lib.lib.kgcn_last_error().decode() == message
        torch.cuda.synchronize()
        for t, b in zip(outs, before):
            np.testing.assert_array_equal(bytes_of(t), b)

    # (a)
    refused(aligned, need - 1, "%s: workspace %d < %d bytes" % (entry, need - 1, need))
    if packed_align is not None and packed_align > 4:
        refused(big[a0 + 4:a0 + 4 + need], need, "%s: workspace not %d-byte aligned" % (entry, packed_align))
    # (b), (c)
    got = []
    for ws in (aligned, skewed) if packed_align is None else (aligned,):
        big.fill_(0xA5)
        if prepare is not None:
            prepare(ws, need)
        outs = outputs()
        assert call(outs, ws, need) == 0, _lib.lib.kgcn_last_error()
        torch.cuda.synchronize()
        got.append([bytes_of(t) for t in outs])
        first = ws.data_ptr() - big.data_ptr()                        # nothing outside the `need` bytes handed in is written
        assert bool((big[:first] == 0xA5).all()) and bool((big[first + need:] == 0xA5).all())
    for b, c in zip(got[0], got[-1]):
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


# ---- the packed layouts of the training step's ops: carved at 4 bytes from the caller's pointer as it is (packed_align) -------------
# One test per multi-array layout, at the smallest shape that uses every array.  Whether the gradients are right is the job of the
# per-family tests, which run the same code with exactly-sized workspaces; here the operands only have to be finite.

def rnd(*shape, seed=0, lo=None):
    """float32 N(0, 1) on the device (lo: uniform in [lo, lo + 1) instead)"""
    rng = np.random.default_rng([seed, len(shape)] + list(shape))
    a = rng.standard_normal(shape) if lo is None else lo + rng.random(shape)
    return up(a.astype(np.float32))


def test_graph_bn():
    import torch
    from kgcn_amd import _lib
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    T, N, d = 2, 3, 5
    x, grad, enabled = rnd(T, N, d), rnd(T, N, d, seed=1), up(np.array([3, 2], np.int32))
    mean, var, gamma = rnd(d, seed=2), rnd(d, lo=0.5), rnd(d, lo=0.5, seed=3)
    need = L.kgcn_graph_bn_workspace_bytes(d)
    vec = lambda: filled((d,), torch.float32)
    contract("kgcn_graph_bn_stats_f32",
             lambda o, ws, nb: L.kgcn_graph_bn_stats_f32(ptr(x), T, N, d, ptr(enabled), ptr(o[0]), ptr(o[1]), ptr(ws), nb, stream()),
             lambda: [vec(), vec()], need, packed_align=8)
    last = []

    def bwd(o, ws, nb):                                               # training with dx: both partial arrays and the count
        last[:] = o
        return L.kgcn_graph_bn_bwd_f32(ptr(x), ptr(grad), T, N, d, ptr(enabled), ptr(mean), ptr(var), ptr(gamma), 1e-3, 1, ptr(o[0]),
                                       ptr(o[1]), ptr(o[2]), ptr(ws), nb, stream())

    contract("kgcn_graph_bn_bwd_f32", bwd, lambda: [filled((T, N, d), torch.float32), vec(), vec()], need, packed_align=8)
    assert all(bool(torch.isfinite(t).all()) for t in last) and not bool((last[0][0] == SENTINEL).any())


def test_ragged_plan():
    """a single array, but of 8-byte words (int2 block sums): the one alignment refusal beside batch normalisation's"""
    import torch
    from kgcn_amd import _lib
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    csr, nn, _ = two_graphs()
    a = csr.desc()
    last = []

    def call(o, ws, nb):
        last[:] = o
        return L.kgcn_ragged_plan(ctypes.byref(a), ptr(nn), None, 2, ptr(o[0]), ptr(o[1]), ptr(ws), nb, stream())

    contract("kgcn_ragged_plan", call, lambda: [filled((3,), torch.int32), filled((3,), torch.int32)],
             L.kgcn_ragged_workspace_bytes(2), packed_align=8)
    assert last[0].tolist() == [0, 3, 5] and last[1].tolist() == [0, 4, 6]      # valid rows and stored entries, scanned


def test_gat():
    import torch
    from kgcn_amd import _lib
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    csr, _, _ = two_graphs()
    d = 3
    x, wa, g = rnd(2, 3, d), rnd(2 * d, seed=1), rnd(2, 3, d, seed=2)
    a, at = csr.desc(), csr.transpose().desc()
    need = L.kgcn_gat_workspace_bytes(2, 3, d)
    contract("kgcn_gat_fwd_f32",
             lambda o, ws, nb: L.kgcn_gat_fwd_f32(ctypes.byref(a), ptr(x), d, ptr(wa), ptr(o[0]), 0.0, ptr(ws), nb, stream()),
             lambda: [filled((2, 3, d), torch.float32)], need, packed_align=4)
    contract("kgcn_gat_bwd_f32",
             lambda o, ws, nb: L.kgcn_gat_bwd_f32(ctypes.byref(a), ctypes.byref(at), ptr(x), d, ptr(wa), ptr(g), ptr(o[0]), 0.0, ptr(o[1]),
                                                  ptr(ws), nb, stream()),
             lambda: [filled((2, 3, d), torch.float32), filled((2 * d,), torch.float32)], need, packed_align=4)


def test_graph_maxpool_bwd():
    import torch
    from kgcn_amd import _lib
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    csr, _, _ = two_graphs()
    d = 3
    x, g = rnd(2, 3, d), rnd(2, 3, d, seed=1)
    a, at = csr.desc(), csr.transpose().desc()
    contract("kgcn_graph_maxpool_bwd_f32",
             lambda o, ws, nb: L.kgcn_graph_maxpool_bwd_f32(ctypes.byref(a), ctypes.byref(at), ptr(x), ptr(g), d, ptr(o[0]), 0.0, ptr(ws),
                                                            nb, stream()),
             lambda: [filled((2, 3, d), torch.float32)], L.kgcn_graph_maxpool_bwd_workspace_bytes(2, 3, d), packed_align=4)


def test_seq_convpool_bwd():
    import torch
    from kgcn_amd import _lib, ops
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    B, length, S, E, k, F, pool = 2, 2, 1, 1, 1, 1, 1                 # the smallest of everything; 2 pooled positions
    ops.seq_limits_check(length=length, symbols=S, embed_dim=E, kernel_size=k, filters=F, pool=pool)
    tokens, table, w, bias = up(np.zeros((B, length), np.int32)), rnd(S, E, lo=0.5), rnd(k, E, F, lo=0.5), rnd(F, lo=0.5)
    out, argmax = filled((B, length // pool, F), torch.float32), filled((B, length // pool, F), torch.uint8)
    assert L.kgcn_seq_convpool_fwd_f32(ptr(tokens), B, length, ptr(table), S, E, ptr(w), ptr(bias), k, F, pool, ptr(out), ptr(argmax),
                                       stream()) == 0
    dout = rnd(B, length // pool, F, seed=1)
    contract("kgcn_seq_convpool_bwd_f32",
             lambda o, ws, nb: L.kgcn_seq_convpool_bwd_f32(ptr(tokens), B, length, ptr(table), S, E, ptr(w), k, F, pool, ptr(dout),
                                                           ptr(argmax), ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(ws), nb, stream()),
             lambda: [filled((S, E), torch.float32), filled((k, E, F), torch.float32), filled((F,), torch.float32)],
             L.kgcn_seq_convpool_workspace_bytes(B, length, S, E, k, F, pool), packed_align=4)


def test_seq_lstm_bwd():
    import torch
    from kgcn_amd import _lib
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    B, steps, D, H = 2, 2, 3, 2
    act = _lib.K["KGCN_SEQ_ACT_HARD_SIGMOID"]
    x, wx, wh, bias, dh = rnd(B, steps, D), rnd(D, 4 * H, seed=1), rnd(H, 4 * H, seed=2), rnd(4 * H, seed=3), rnd(B, H, seed=4)
    h, stash = filled((B, H), torch.float32), filled((int(L.kgcn_seq_lstm_stash_floats(B, steps, H)),), torch.float32)
    assert L.kgcn_seq_lstm_fwd_f32(ptr(x), B, steps, D, ptr(wx), ptr(wh), ptr(bias), H, act, ptr(h), H, ptr(stash), stream()) == 0
    keep = []

    def call(o, ws, nb):                                              # the backward overwrites the stash: every call gets a copy
        keep[:] = [stash.clone()]
        return L.kgcn_seq_lstm_bwd_f32(ptr(x), B, steps, D, ptr(wx), ptr(wh), ptr(bias), H, act, ptr(dh), H, ptr(keep[0]), ptr(o[0]),
                                       ptr(o[1]), ptr(o[2]), ptr(o[3]), ptr(ws), nb, stream())

    contract("kgcn_seq_lstm_bwd_f32", call,
             lambda: [filled((B, steps, D), torch.float32), filled((D, 4 * H), torch.float32), filled((H, 4 * H), torch.float32),
                      filled((4 * H,), torch.float32)], L.kgcn_seq_lstm_workspace_bytes(B, steps, D, H), packed_align=4)


def test_conv1d_pool_bwd():
    import torch
    from kgcn_amd import _lib, ops
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    B, length, Cin, k, F, pool = 2, 2, 1, 1, 1, 1                     # the smallest of everything; 2 pooled positions
    ops.conv1d_limits_check(length=length, in_dim=Cin, filters=F, kernel_size=k, pool=pool)
    act = _lib.K["KGCN_ACT_RELU"]
    x, w, bias = rnd(B, length, Cin, lo=0.5), rnd(k, Cin, F, lo=0.5), rnd(F, lo=0.5)
    out, argmax = filled((B, length // pool, F), torch.float32), filled((B, length // pool, F), torch.uint8)
    assert L.kgcn_conv1d_pool_fwd_f32(ptr(x), None, None, 0, B, length, Cin, ptr(w), ptr(bias), k, F, pool, act, ptr(out), ptr(argmax),
                                      stream()) == 0
    dout = rnd(B, length // pool, F, seed=1)
    contract("kgcn_conv1d_pool_bwd_f32",                              # dx and dw: the flipped weights and both partial arrays
             lambda o, ws, nb: L.kgcn_conv1d_pool_bwd_f32(ptr(x), None, None, 0, B, length, Cin, ptr(w), k, F, pool, act, ptr(dout),
                                                          ptr(argmax), ptr(out), ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(ws), nb, stream()),
             lambda: [filled((B, length, Cin), torch.float32), filled((k, Cin, F), torch.float32), filled((F,), torch.float32)],
             L.kgcn_conv1d_pool_workspace_bytes(B, length, Cin, k, F, pool), packed_align=4)


def test_cpi_ig():
    import torch
    from kgcn_amd import _lib
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    C, N, Wd, T, K = 2, 2, 3, 2, 2
    P, Q, u, e = rnd(C, N, Wd), rnd(C, N, Wd, seed=1), rnd(T, Wd, seed=2), rnd(T, seed=3)
    alpha, gamma, wA, wB = (up(np.array(v, np.float32)) for v in ([0.0, 1.0], [1.0, 1.0], [0.5, 0.5], [0.25, 0.75]))
    contract("kgcn_cpi_ig_f32",
             lambda o, ws, nb: L.kgcn_cpi_ig_f32(ptr(P), ptr(Q), C, N, Wd, ptr(u), ptr(e), T, ptr(alpha), ptr(gamma), ptr(wA), ptr(wB), K,
                                                 ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(ws), nb, stream()),
             lambda: [filled((C, K, T), torch.float32), filled((C, T, N, Wd), torch.float32), filled((C, T, N, Wd), torch.float32)],
             L.kgcn_cpi_ig_workspace_bytes(C, Wd, T, K), packed_align=4)


def test_vae_recon_bwd():
    import torch
    from kgcn_amd import _lib, ops
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    csr, _, _ = two_graphs()
    B, N, C, d, f = 2, 3, 2, 1, 1                                     # d = 1: the smallest decoder width recon_args admits
    adj = (_lib.CsrBatch * C)(csr.desc(), csr.desc())
    ys, ws_ = [rnd(B, N, d, seed=c) for c in range(C)], [rnd(d, lo=0.5, seed=c) for c in range(C)]
    logits, target, g_opt = rnd(B, N, f, seed=5), rnd(B, N, f, lo=0.0, seed=6), up(np.ones(1, np.float32))
    contract("kgcn_vae_recon_bwd_f32",                                # dw of both channels
             lambda o, ws, nb: L.kgcn_vae_recon_bwd_f32(adj, C, ops._ptr_array(ys), ops._ptr_array(ws_), d, ptr(logits), ptr(target), f,
                                                        None, ptr(g_opt), None, ops._ptr_array(o[0:2]), ops._ptr_array(o[2:4]), ptr(o[4]),
                                                        None, ptr(ws), nb, stream()),
             lambda: [filled((B, N, d), torch.float32) for _ in range(C)] + [filled((d,), torch.float32) for _ in range(C)] +
                     [filled((B, N, f), torch.float32)], L.kgcn_vae_recon_workspace_bytes(B, C, d), packed_align=4)


def test_dense_wgrad():
    import torch
    from kgcn_amd import _lib
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    m, din, dout = 5, 3, 2
    x, dy = rnd(m, din), rnd(m, dout, seed=1)
    contract("kgcn_dense_wgrad_f32",
             lambda o, ws, nb: L.kgcn_dense_wgrad_f32(ptr(x), din, ptr(dy), dout, m, din, dout, ptr(o[0]), ptr(o[1]), ptr(ws), nb, stream()),
             lambda: [filled((din, dout), torch.float32), filled((dout,), torch.float32)],
             L.kgcn_dense_wgrad_workspace_bytes(m, din, dout), packed_align=4)


def test_dense_bwd_and_bwd_dot():
    import torch
    from kgcn_amd import _lib
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    m, din, dout = 16384, 132, 256                                    # the smallest shape kgcn_dense_bwd_supported admits
    assert L.kgcn_dense_bwd_supported(m, din, dout) and not L.kgcn_dense_bwd_supported(m - 1, din, dout)
    assert not L.kgcn_dense_bwd_supported(m, din - 4, dout)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x, grad, dotx = (torch.randn((m, n), device="cuda", generator=gen) for n in (din, dout, din))
    act_out = torch.rand((m, dout), device="cuda", generator=gen)
    w = torch.randn((din, dout), device="cuda", generator=gen) / 16
    act = _lib.K["KGCN_ACT_SIGMOID"]
    tb = L.kgcn_dense_fwd_workspace_bytes(dout, din)
    table = torch.empty((tb,), device="cuda", dtype=torch.uint8)
    need = L.kgcn_dense_wgrad_workspace_bytes(m, din, dout)
    grads = lambda: [filled((din, dout), torch.float32), filled((dout,), torch.float32)]
    contract("kgcn_dense_bwd_f32",
             lambda o, ws, nb: L.kgcn_dense_bwd_f32(ptr(grad), None, 0, 0, ptr(act_out), act, dout, ptr(x), din, m, din, dout, ptr(w), dout,
                                                    ptr(o[2]), din, ptr(o[0]), ptr(o[1]), ptr(table), tb, 0, ptr(ws), nb, stream()),
             lambda: grads() + [filled((m, din), torch.float32)], need, packed_align=4)
    contract("kgcn_dense_bwd_dot_f32",
             lambda o, ws, nb: L.kgcn_dense_bwd_dot_f32(ptr(grad), ptr(act_out), act, dout, ptr(x), din, m, din, dout, ptr(w), dout,
                                                        ptr(dotx), din, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(table), tb, 0, ptr(ws), nb,
                                                        stream()),
             lambda: grads() + [filled((1,), torch.float32)], need, packed_align=4)


def test_graphconv_bwd():
    import torch
    import fused_cases
    from kgcn_amd import BatchedCSR, _lib, ops
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    name = min(fused_cases.FULL_CASES + fused_cases.PACK_CASES, key=lambda n: np.prod(fused_cases.shape_of(n)))
    T = 2
    N, din, dout = fused_cases.shape_of(name)
    case = fused_cases.build(name, T)
    csr = BatchedCSR.from_arrays(case.graph, case.row, case.col, case.val, T, N, N, device="cuda")
    at = ops._fused_adjacency(csr.transpose(), True, T, din, dout, True)
    x, w, g = rnd(T, N, din), rnd(din, dout, seed=1), rnd(T, N, dout, seed=2)
    contract("kgcn_graphconv_bwd_f32",                                # one partial pair per workgroup, at most one workgroup a graph
             lambda o, ws, nb: L.kgcn_graphconv_bwd_f32(at, ptr(x), ptr(w), ptr(g), din, dout, ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(ws), nb,
                                                        stream()),
             lambda: [filled((T, N, din), torch.float32), filled((din, dout), torch.float32), filled((dout,), torch.float32)],
             L.kgcn_graphconv_bwd_workspace_bytes(T, din, dout), exact=False, packed_align=4)


def test_gcn_stack_bwd():
    import torch
    import stack_cases
    from kgcn_amd import _lib, ops
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream
    csr, nn, _ = two_graphs()
    name = min(stack_cases.CASES, key=lambda n: (len(stack_cases.CASES[n]["widths"]), sum(stack_cases.CASES[n]["widths"])))
    spec = stack_cases.spec_of(name)
    assert ops.gcn_stack_supported(csr, spec)
    T, N = 2, 3
    params = []
    for l, (kind, act, din, dout, eps) in enumerate(spec):
        assert kind != 2                                              # (a list with a normalisation would need its buffers here)
        params += [rnd(din, dout, seed=l) / np.sqrt(din), rnd(dout, seed=10 + l)]
    arr, keep = ops._stack_descriptors(spec, params, [None] * len(spec))
    x, dlast = rnd(T, N, spec[0][2]), rnd(T, spec[-1][3], seed=1)
    outs = [filled((T, N, s[3]), torch.float32) for s in spec]
    optr = (ctypes.c_void_p * len(spec))(*[o.data_ptr() for o in outs])
    pooled = filled((T, spec[-1][3]), torch.float32)
    assert L.kgcn_gcn_stack_fwd_f32(ctypes.byref(csr.desc()), ptr(x), ptr(nn), arr, len(spec), optr, ptr(pooled), stream()) == 0
    at = csr.transpose().desc()
    n = int(L.kgcn_gcn_stack_param_floats(arr, len(spec)))
    contract("kgcn_gcn_stack_bwd_f32",
             lambda o, ws, nb: L.kgcn_gcn_stack_bwd_f32(ctypes.byref(at), ptr(x), ptr(nn), arr, len(spec), optr, ptr(dlast), 1, ptr(o[0]),
                                                        ptr(o[1]), ptr(ws), nb, stream()),
             lambda: [filled((T, N, spec[0][2]), torch.float32), filled((n,), torch.float32)],
             L.kgcn_gcn_stack_bwd_workspace_bytes(T, arr, len(spec)), exact=False, packed_align=4)
