"""Every op of kgcn_amd/csrc/graphkern.hip on its own, on the cases of tests/graph_kernel_cases.py and against the plain references
there (the Weisfeiler-Lehman partitions and Grams of the graph set against tests/graph_kernel_oracle.py): the OUTPUTS of the ops
as include/kgcn_hip.h states them -- run lists with their order, run_ptr and capacity, sorted_nbr, the key classes, the plan's
statistics -- and not only the Gram they end in.  tests/test_gpu_graph_kernel.py holds the two public functions to the fixture;
this file goes where that one does not: five tile rows of the Gram and the chunk edges, wl_runs up to its 4,096 rows, a refinement
of 62,400 rows with degrees of 299, the bitonic network of the shortest-path kernel at and around its powers of two, label rank
4,095, a directed CSR.  Every comparison is exact (assert_array_equal), every op runs twice and must repeat itself byte for byte.

An entry whose column is no node of its graph: kgcn_sp_features_i32 ignores it (the `directed` case), kgcn_wl_refine_i32 counts it
as a neighbour of colour -1 (test_wl_refine_on_a_directed_csr); the head of graphkern.hip says so, and these two tests hold it."""
import ctypes
import functools
import re

import numpy as np
import pytest

import graph_kernel_cases as C
import graph_kernel_oracle as O

pytestmark = pytest.mark.gpu

SENTINEL = -7


def up(a):
    """to the device; the cases' arrays are read-only and shared between tests: upload a copy"""
    import torch
    return torch.from_numpy(np.array(a)).to("cuda")


def host(t):
    return t.cpu().numpy()


def same_bytes(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    np.testing.assert_array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def twice(op):
    """the op's outputs on the host, after a second call has given the same bytes"""
    first, second = [[host(t) for t in op()] for _ in range(2)]
    for a, b in zip(first, second):
        same_bytes(a, b)
    return first


def csr_of(entries, T, M):
    from kgcn_amd.batched_csr import BatchedCSR
    g, r, c = entries
    return BatchedCSR.from_arrays(g, r, c, np.ones(len(g), np.float32), T, M, M)


def same_runs(got, ref, T):
    """(col, graph, count) against the reference's (run_ptr, col, graph, count); run_ptr as the graph column implies it"""
    ptr, col, graph, count = ref
    assert [a.dtype for a in got] == [np.int64, np.int32, np.int32]
    np.testing.assert_array_equal(got[1], graph)
    np.testing.assert_array_equal(np.concatenate([[0], np.cumsum(np.bincount(got[1], minlength=T))]), ptr)
    np.testing.assert_array_equal(got[0], col)
    np.testing.assert_array_equal(got[2], count)


def integers(K):
    assert K.dtype == np.float64 and np.all(K == np.rint(K)) and np.abs(K).max(initial=0) < 2.0 ** 53
    return K.astype(np.int64)


# ---- 1. Gram from synthetic runs -------------------------------------------------------------------------------------------------
NORMALISED = "g260_c16_d50"                                         # has graphs with a zero diagonal


@pytest.mark.parametrize("name", C.GRAM_NAMES)
def test_gram_from_synthetic_runs(name):
    from kgcn_amd import ops
    case = C.gram_case(name)
    G, chunk_cols, _ = case.spec
    col, graph, count = up(case.col), up(case.graph), up(case.count)
    seen = []

    def op():
        K, stats = ops.gram_from_runs(col, graph, count, G, chunk_cols=chunk_cols, return_stats=True)
        seen.append((stats["columns"], stats["diag_columns"], stats["dense_columns"]))
        return [K]

    K, = twice(op)
    assert seen == [case.stats, case.stats]
    assert K.shape == (G, G)
    np.testing.assert_array_equal(integers(K), case.K)
    np.testing.assert_array_equal(K, K.T)
    for a, b in ((col, case.col), (graph, case.graph), (count, case.count)):           # the runs are read, not reordered in place
        np.testing.assert_array_equal(host(a), b)
    if name == NORMALISED:
        assert case.empty and not case.K[list(case.empty)].any()
        norm, = twice(lambda: [ops.gram_from_runs(col, graph, count, G, chunk_cols=chunk_cols, normalize=True)])
        same_bytes(norm, O.normalize(case.K))


# ---- 2. wl_runs on synthetic colours ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", C.WL_RUNS_M)
def test_wl_runs_on_synthetic_colours(M):
    from kgcn_amd import ops
    case = C.wl_runs_case(M)
    colours, nn = up(case.colours.reshape(-1)), up(case.num_nodes)
    got = twice(lambda: ops.wl_runs(colours, nn, case.T, M, C.WL_RUNS_OFFSET))
    same_runs(got, case.runs, case.T)


# ---- 3. refinement and ranking of 62,400 rows ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_wl_set():
    from kgcn_amd import graph_kernel as gk
    s = C.wl_set()
    adjs, nn, lab = O.to_adjs(list(s.graphs), C.WL_M)
    return gk.GraphSet(adjs, nn, lab), nn


def test_wl_set_colours_are_the_oracle_partition_after_every_iteration():
    from kgcn_amd import graph_kernel as gk, ops
    s = C.wl_set()
    gs, nn = device_wl_set()
    assert (gs.T, gs.M) == (len(s.graphs), C.WL_M) == (208, 300)
    cols, _ = gk.wl_colourings(gs, iterations=C.WL_ITERATIONS)
    col, _ = gs.initial_colours("node")                              # the same steps by hand: info, and the second call
    by_hand = [col]
    for it in range(C.WL_ITERATIONS):
        sorted_nbr, hi, lo = ops.wl_refine(gs.csr, gs.num_nodes, col)
        col, info = ops.wl_rank(gs.csr, gs.num_nodes, col, sorted_nbr, hi, lo)
        assert host(info).tolist() == [len(set(s.colours[it + 1].tolist())), 0], it
        by_hand.append(col)
    exists = np.arange(C.WL_M)[None, :] < nn[:, None]
    tri, hexa = s.index["triangles"], s.index["hexagon"]
    for it, (c, h, ref) in enumerate(zip(cols, by_hand, s.colours)):
        c = host(c)
        same_bytes(c, host(h).reshape(c.shape))
        assert c.dtype == np.int32 and c.shape == (208, 300)
        assert np.all(c[~exists] == -1) and np.all(c[exists] >= 0), it
        mine = c[exists]                                              # row-major: the oracle's concatenation order
        np.testing.assert_array_equal(O.first_occurrence(mine), O.first_occurrence(ref), err_msg="iteration %d" % it)
        assert np.array_equal(np.unique(mine), np.arange(len(set(ref.tolist())))), it    # dense ids
        np.testing.assert_array_equal(np.sort(c[tri, :6]), np.sort(c[hexa, :6]), err_msg="iteration %d" % it)


def test_wl_set_gram_and_plan_statistics():
    from kgcn_amd import graph_kernel as gk, ops
    import torch
    s = C.wl_set()
    gs, _ = device_wl_set()
    K, = twice(lambda: [gk.wl_subtree_kernel(gs, iterations=C.WL_ITERATIONS, normalize=False)])
    np.testing.assert_array_equal(integers(K), s.gram)
    np.testing.assert_array_equal(K, K.T)
    cols, _ = gk.wl_colourings(gs, iterations=C.WL_ITERATIONS)       # the same route taken apart, for the statistics
    runs = [ops.wl_runs(c.reshape(-1), gs.num_nodes, gs.T, gs.M, it << 32) for it, c in enumerate(cols)]
    col, graph, count = (torch.cat([r[i] for r in runs]) for i in range(3))
    K2, stats = ops.gram_from_runs(col, graph, count, gs.T, return_stats=True)
    assert (stats["columns"], stats["diag_columns"], stats["dense_columns"]) == s.columns
    same_bytes(host(K2), K)


def test_wl_refine_on_a_directed_csr():
    """sorted_nbr and the key classes of ops.wl_refine, then wl_rank on them; an entry whose column is no node of its graph counts
    in the degree and enters the list with the colour -1 (rows (5, 0) and (5, 1) of the case differ in nothing else)"""
    from kgcn_amd import ops
    d = C.wl_direct()
    csr = csr_of(d.entries, d.T, d.M)
    nn, colours = up(d.num_nodes), up(d.colours.reshape(-1))
    sorted_nbr, hi, lo = twice(lambda: ops.wl_refine(csr, nn, colours))
    assert csr.nnz == len(d.sorted_nbr)
    np.testing.assert_array_equal(sorted_nbr[:csr.nnz], d.sorted_nbr)
    exists = (np.arange(d.M)[None, :] < d.num_nodes[:, None]).reshape(-1)
    assert hi.shape == lo.shape == (d.T * d.M,)
    assert np.all(hi[~exists] == -1) and np.all(lo[~exists] == -1)  # all ones
    keys = list(zip(hi[exists].tolist(), lo[exists].tolist()))
    ids = {}
    np.testing.assert_array_equal(O.first_occurrence([ids.setdefault(k, len(ids)) for k in keys]),
                                  O.first_occurrence(d.classes.reshape(-1)[exists]))     # equal keys iff one class
    (ta, ra), (tb, rb) = d.pad_rows
    assert keys[int(exists[:ta * d.M + ra].sum())] != keys[int(exists[:tb * d.M + rb].sum())]
    t_sorted, t_hi, t_lo = ops.wl_refine(csr, nn, colours)
    new, info = twice(lambda: ops.wl_rank(csr, nn, colours, t_sorted, t_hi, t_lo))
    assert info.tolist() == [len(set(d.classes.reshape(-1)[exists].tolist())), 0]
    assert np.all(new[~exists] == -1)
    np.testing.assert_array_equal(O.first_occurrence(new[exists]), O.first_occurrence(d.classes.reshape(-1)[exists]))


# ---- 4. shortest-path features ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.SP_NAMES)
def test_sp_features_runs(name):
    from kgcn_amd import ops
    case = C.sp_case(name)
    csr = csr_of(case.entries, case.T, case.M)
    nn, labels = up(case.num_nodes), up(case.labels.reshape(-1))
    got = twice(lambda: ops.sp_features(csr, nn, labels, case.num_labels))
    same_runs(got, case.runs, case.T)


# ---- 5. never past the capacity --------------------------------------------------------------------------------------------------
def two_passes_and_a_short_one(call, T, ref):
    """call(run_ptr, col, graph, count, capacity, ws, ws_bytes) -> rc of the C entry point: the count pass, the emit pass, and the
    emit pass again with three entries less than it needs into buffers that hold a sentinel"""
    import torch
    from kgcn_amd import _lib
    L, ptr = _lib.lib, _lib.ptr
    need = L.kgcn_graph_runs_workspace_bytes(T)
    assert need > 0
    ws = torch.empty((need,), device="cuda", dtype=torch.uint8)
    run_ptr = torch.full((T + 1,), SENTINEL, device="cuda", dtype=torch.int64)
    assert call(ptr(run_ptr), None, None, None, 0, ptr(ws), need) == 0, L.kgcn_last_error()
    np.testing.assert_array_equal(host(run_ptr), ref[0])
    total = int(ref[0][-1])
    assert total > 3

    def buffers():
        return [torch.full((total,), SENTINEL, device="cuda", dtype=dt) for dt in (torch.int64, torch.int32, torch.int32)]

    full, short = buffers(), buffers()
    assert call(ptr(run_ptr), ptr(full[0]), ptr(full[1]), ptr(full[2]), total, ptr(ws), need) == 0, L.kgcn_last_error()
    assert call(ptr(run_ptr), ptr(short[0]), ptr(short[1]), ptr(short[2]), total - 3, ptr(ws), need) == 0, L.kgcn_last_error()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host(run_ptr), ref[0])             # the emit pass reads it
    for f, s, r in zip(full, short, ref[1:]):
        f, s = host(f), host(s)
        np.testing.assert_array_equal(f, r)
        np.testing.assert_array_equal(s[:total - 3], r[:total - 3])
        assert np.all(s[total - 3:] == SENTINEL)


@pytest.mark.parametrize("op", ["wl_runs", "sp_features"])
def test_runs_are_never_written_past_the_capacity(op):
    from kgcn_amd import _lib
    L, ptr, stream = _lib.lib, _lib.ptr, _lib.current_stream()
    if op == "wl_runs":
        case = C.wl_runs_case(1000)
        colours, nn = up(case.colours.reshape(-1)), up(case.num_nodes)
        two_passes_and_a_short_one(lambda rp, c, g, n, cap, ws, wsb: L.kgcn_wl_runs_i32(
            ptr(colours), ptr(nn), case.T, case.M, C.WL_RUNS_OFFSET, rp, c, g, n, cap, ws, wsb, stream), case.T, case.runs)
    else:
        case = C.sp_case("m128")
        csr = csr_of(case.entries, case.T, case.M)
        nn, labels = up(case.num_nodes), up(case.labels.reshape(-1))
        two_passes_and_a_short_one(lambda rp, c, g, n, cap, ws, wsb: L.kgcn_sp_features_i32(
            ctypes.byref(csr.desc()), ptr(nn), ptr(labels), case.num_labels, rp, c, g, n, cap, ws, wsb, stream), case.T, case.runs)


# ---- 6. refusals before any launch -----------------------------------------------------------------------------------------------
def refused(rc, pattern, query=False):
    from kgcn_amd import _lib
    assert rc == (-1 if query else 1), rc
    msg = _lib.lib.kgcn_last_error().decode()
    assert re.search(pattern, msg), msg


def test_refusals_name_their_reason_before_any_launch():
    """Return code and kgcn_last_error of what the entry points refuse.  Where the refusal comes first no operand exists (NULL);
    where operands are checked before it they are real and sized for the call, so that a refusal that went missing would still
    stay inside them."""
    import torch
    from kgcn_amd import _lib
    L, ptr = _lib.lib, _lib.ptr
    refused(L.kgcn_wl_runs_i32(None, None, 1, 4097, 0, None, None, None, None, 0, None, 0, None), r"4097 rows a graph, up to 4096")
    for cc in (8, 24, (1 << 20) + 16):
        refused(L.kgcn_graph_gram_workspace_bytes(10, 4, cc), r"chunk_cols %d must be a multiple of 16" % cc, query=True)
        refused(L.kgcn_gram_plan_i64(None, None, None, 10, 4, cc, None, None, 0, None), r"chunk_cols %d must be a multiple of 16" % cc)
        refused(L.kgcn_gram_dense_f64(None, None, 10, 4, 0, cc, None, None, 0, None), r"chunk_cols %d must be a multiple of 16" % cc)
    assert L.kgcn_graph_gram_workspace_bytes(10, 46340, 16) > 0
    refused(L.kgcn_graph_gram_workspace_bytes(10, 46341, 16), r"46341 graphs outside 1\.\.46,340", query=True)
    # dense_cols > runs / 2, after a real plan of four runs in one dense and two diag columns
    col, graph, count = up(np.array([9, 9, 4, 5], np.int64)), up(np.array([0, 1, 0, 1], np.int32)), up(np.array([1, 2, 3, 4], np.int32))
    need = L.kgcn_graph_gram_workspace_bytes(4, 2, 16)
    ws = torch.empty((need,), device="cuda", dtype=torch.uint8)
    stats = torch.zeros((3,), device="cuda", dtype=torch.int64)
    K = torch.full((2, 2), float(SENTINEL), device="cuda", dtype=torch.float64)
    assert L.kgcn_gram_plan_i64(ptr(col), ptr(graph), ptr(count), 4, 2, 16, ptr(stats), ptr(ws), need, None) == 0
    assert host(stats).tolist() == [3, 2, 1]
    refused(L.kgcn_gram_dense_f64(ptr(graph), ptr(count), 4, 2, 3, 16, ptr(K), ptr(ws), need, None), r"3 dense columns for 4 runs")
    assert np.all(host(K) == SENTINEL)
    assert L.kgcn_gram_dense_f64(ptr(graph), ptr(count), 4, 2, 1, 16, ptr(K), ptr(ws), need, None) == 0
    np.testing.assert_array_equal(host(K), [[1 + 9, 2], [2, 4 + 16]])
    # run_col without run_graph; a count-mode workspace one byte short
    colours, nn = up(np.zeros(1, np.int32)), up(np.ones(1, np.int32))
    need = L.kgcn_graph_runs_workspace_bytes(1)
    ws = torch.empty((need,), device="cuda", dtype=torch.uint8)
    run_ptr = torch.full((2,), SENTINEL, device="cuda", dtype=torch.int64)
    run_col = torch.full((1,), SENTINEL, device="cuda", dtype=torch.int64)
    refused(L.kgcn_wl_runs_i32(ptr(colours), ptr(nn), 1, 1, 0, ptr(run_ptr), ptr(run_col), None, None, 0, ptr(ws), need, None),
            r"run_col without run_graph")
    refused(L.kgcn_wl_runs_i32(ptr(colours), ptr(nn), 1, 1, 0, ptr(run_ptr), None, None, None, 0, ptr(ws), need - 1, None),
            r"workspace %d < %d bytes" % (need - 1, need))
    torch.cuda.synchronize()
    assert np.all(host(run_ptr) == SENTINEL) and np.all(host(run_col) == SENTINEL)
    assert L.kgcn_wl_runs_i32(ptr(colours), ptr(nn), 1, 1, 0, ptr(run_ptr), None, None, None, 0, ptr(ws), need, None) == 0
    assert host(run_ptr).tolist() == [0, 1]
