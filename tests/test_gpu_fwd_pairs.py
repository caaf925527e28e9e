"""The FULL-shape fused GraphConv forward (N = 32, din = dout = 64) as reader | aggregator wave pairs (graphconv_fwd_full_kernel).

From T0 graphs on, and while two CSR slices per pair fit the LDS, kgcn_graphconv_fwd_f32 runs the forward as four wave pairs per
workgroup: one wave reads x and the CSR slice and multiplies, the other aggregates the graph before and stores it, one workgroup
barrier per graph.  Shorter batches and larger slices keep one wave per graph (graphconv_fwd_wave_kernel).  Both compute the same
bits.  The 1,024 pairs of a launch own ceil(T / 1024) or one graph less: T0 + 1,023 leaves some pairs a graph short, 18,432 makes
every pair whole.  Checked here: the route query, the sizes around T0 in the three adjacency layouts against the fp64 oracle, bit equality
with the one-wave kernel (the same entry point on slices shorter than T0, a non-zero bias), that every element of the output is
written and nothing else, directed / long-row / > 256-entry / empty-row graphs, and a captured replay.

Reference (fp64 numpy) and tolerances are those of tests/test_gpu_fused_ingest.py and tests/test_gpu_fused_cases.py; nothing is
compared more loosely here.  (tests/family_bounds.py holds no bound for the fused GraphConv family: its tolerance is the written
form atol 1e-5 + 1e-6 max|ref| of test_graphconv_fused.)
"""
import functools

import numpy as np
import pytest
import torch

import fused_cases as F
from oracle import kgcn_oracle as K
from test_gpu_parity import close, dev, t32

pytestmark = pytest.mark.gpu

N, D = 32, 64
T0 = 16384                      # fused.hip: KGCN_FWD_PAIRS_MIN_GRAPHS (profiles/fwd_pairs_ab.txt)
PAIRS = 4 * 256                 # wave pairs of a launch
WHOLE = 3 * 1024 * 6            # the first multiple of 3 * 1,024 that is >= T0: every pair owns eighteen graphs
SIZES = [T0 - 1, T0, T0 + 1, T0 + 1023, WHOLE]
COMPACT = 0x104
GUARD = 4096                    # floats in front of and behind the output (16 KiB each: two tiles)
FILL = 0x7fc0a5a5               # a quiet NaN with a payload no kernel produces


def test_sizes_name_the_edges():
    assert WHOLE >= T0 and WHOLE % PAIRS == 0 and WHOLE - 3 * 1024 < T0
    assert (T0 + 1023) % PAIRS != 0 and (T0 + 1023) // PAIRS >= 2


def route(T, max_nnz):
    from kgcn_amd._lib import lib
    return lib.kgcn_graphconv_fwd_pairs_route(T, N, D, D, max_nnz)


@functools.lru_cache(maxsize=2)
def batch(T, normalize):
    """synthetic molecule graphs with their operands and the fp64 forward, computed once per (T, normalize)"""
    rng = np.random.default_rng(15485863 * T + int(normalize))
    adjs = K.synth_mol_graphs(rng, T, N, 3, normalize=normalize)
    x = rng.standard_normal((T, N, D)).astype(np.float32)
    w = K.glorot_uniform(rng, D, D)
    b = rng.standard_normal((1, D)).astype(np.float32)          # non-zero: the accumulators start from it
    ref = K.graphconv_fwd_fast(x, adjs, [w], [b])
    for a in (x, w, b):
        a.setflags(write=False)
    return adjs, x, w, b, ref


def container(adjs):
    from kgcn_amd import BatchedCSR
    return BatchedCSR.from_coo_list([a[0] for a in adjs], rows=N, cols=N, device=dev())


def c_fwd(desc, x, w, b, out=None):
    from kgcn_amd._lib import check, current_stream, lib, ptr
    out = torch.full_like(x, float("nan")) if out is None else out
    check(lib.kgcn_graphconv_fwd_f32(desc, ptr(x), ptr(w), ptr(b), D, D, ptr(out), current_stream()), "kgcn_graphconv_fwd_f32")
    return out


def descriptor(csr, layout, T):
    """the descriptor of `layout`: the compact copy the layer passes (unit: no value stream, kipf: with one) or the row-padded one"""
    from kgcn_amd import ops
    if layout == "pad4":
        return csr.padded4().desc()
    desc = ops._fused_adjacency(csr, False, T, D, D, False)
    assert desc.row_pad == COMPACT
    return desc


def up(a):
    """to the device; the batch's arrays are read-only and shared between tests: upload a copy"""
    return t32(np.array(a))


def bits(t):
    return t.contiguous().view(torch.int32)


def test_route_query():
    for T in (1, 2047, 2048, 8192, T0 - 1):
        assert route(T, 128) == 0, "T = %d takes the pairs kernel below the threshold" % T
    for T in (T0, T0 + 1, T0 + 1023, WHOLE, 100000):
        assert route(T, 128) == 1, "T = %d does not take the pairs kernel" % T
    assert route(100000, 1024) == 0                  # two slices of 1,024 entries per pair do not fit the LDS
    from kgcn_amd._lib import lib
    assert lib.kgcn_graphconv_fwd_pairs_route(100000, 16, D, D, 128) == 0 and lib.kgcn_graphconv_fwd_pairs_route(100000, N, 32, D, 128) == 0


@pytest.mark.parametrize("layout", ["unit", "kipf", "pad4"])
@pytest.mark.parametrize("T", SIZES)
def test_sizes_around_the_threshold(T, layout):
    adjs, x, w, b, ref = batch(T, layout != "unit")
    csr = container(adjs)
    p4 = csr.padded4()
    assert route(T, p4.max_nnz) == int(T >= T0)
    c4 = p4.compact4()
    assert c4 is not None and c4.unit_values == (layout == "unit")
    out = c_fwd(descriptor(csr, layout, T), up(x), up(w), up(b).reshape(-1))
    close(out, ref, rel=1e-6, what="fused fwd, T = %d, %s" % (T, layout))


@pytest.mark.parametrize("layout", ["unit", "kipf", "pad4"])
def test_bit_equal_to_the_one_wave_kernel(layout):
    """the same batch through the same entry point in slices of fewer than T0 graphs (the one-wave kernel) and in one launch"""
    T = T0 + 1023
    adjs, x, w, b, _ = batch(T, layout != "unit")
    tx, tw, tb = up(x), up(w), up(b).reshape(-1)
    assert float(tb.abs().min()) > 0
    csr = container(adjs)
    assert route(T, csr.padded4().max_nnz) == 1
    whole = c_fwd(descriptor(csr, layout, T), tx, tw, tb)
    step = 6000
    for s in range(0, T, step):
        e = min(T, s + step)
        part = container(adjs[s:e])
        assert route(e - s, part.padded4().max_nnz) == 0
        piece = c_fwd(descriptor(part, layout, e - s), tx[s:e].contiguous(), tw, tb)
        assert torch.equal(bits(piece), bits(whole[s:e])), "graphs %d..%d differ between the pairs and the one-wave kernel" % (s, e)


@pytest.mark.parametrize("T", [T0 + 1, T0 + 1023])
def test_written_once_inside_guards(T):
    adjs, x, w, b, ref = batch(T, True)
    csr = container(adjs)
    desc = descriptor(csr, "kipf", T)
    assert route(T, csr.padded4().max_nnz) == 1
    tx, tw, tb = up(x), up(w), up(b).reshape(-1)

    def launch():
        buf = torch.full((GUARD + T * N * D + GUARD,), FILL, dtype=torch.int32, device=dev())
        out = buf[GUARD:GUARD + T * N * D].view(torch.float32).view(T, N, D)
        assert out.data_ptr() == buf.data_ptr() + 4 * GUARD and out.data_ptr() % 16 == 0
        c_fwd(desc, tx, tw, tb, out)
        torch.cuda.synchronize()
        return buf, out

    buf, out = launch()
    front, back = buf[:GUARD], buf[GUARD + T * N * D:]
    assert int((front != FILL).sum()) == 0, "%d words in front of the output were written" % int((front != FILL).sum())
    assert int((back != FILL).sum()) == 0, "%d words behind the output were written" % int((back != FILL).sum())
    left = buf[GUARD:GUARD + T * N * D] == FILL
    assert int(left.sum()) == 0, "%d elements of the output were not written (first at flat index %d)" % (
        int(left.sum()), int(torch.nonzero(left)[0]))
    close(out, ref, rel=1e-6, what="fused fwd inside guards, T = %d" % T)
    buf2, _ = launch()
    assert torch.equal(buf, buf2), "the output (or a guard word) differs between two launches on the same operands"


@functools.lru_cache(maxsize=1)
def tiled(name):
    """the five graphs of fused_cases.build(name, 5) (graphs 0 and 4 are empty) repeated up to T0 + 1 graphs, fresh operands, and
    the fp64 forward from the dense adjacency"""
    T = T0 + 1
    case = F.build(name, 5)
    reps = (T + 4) // 5
    n = case.graph.shape[0]
    graph = (np.tile(case.graph, reps) + 5 * np.repeat(np.arange(reps), n)).astype(np.int64)
    keep = graph < T
    row, col, val = (np.tile(a, reps)[keep] for a in (case.row, case.col, case.val))
    graph = graph[keep]
    rng = np.random.default_rng([T, len(name)])
    x = rng.standard_normal((T, N, D)).astype(np.float32)
    w = K.glorot_uniform(rng, D, D)
    b = rng.standard_normal((1, D)).astype(np.float32)
    dense = np.tile(case.dense, (reps, 1, 1))[:T]
    ref = np.matmul(dense, np.matmul(x.astype(np.float64), w.astype(np.float64)) + b.astype(np.float64).reshape(1, 1, -1))
    return case, (graph, row, col, val), x, w, b, ref


# directed: A != A^T, empty rows, a row of 20 entries (grp_tail); row64: a row of 64; edge224: 224 row-padded entries;
# k12, row252: more than 256 row-padded entries (the rare landing loops of land_csr_c / land_csr); complete: the one-wave route
@pytest.mark.parametrize("name", ["directed", "directed_unit", "row64", "edge224", "k12", "row252", "complete"])
def test_graph_shapes(name):
    from kgcn_amd import BatchedCSR
    T = T0 + 1
    case, (graph, row, col, val), x, w, b, ref = tiled(name)
    csr = BatchedCSR.from_arrays(graph, row, col, val, T, N, N, device=dev())
    p4 = csr.padded4()
    assert p4.max_nnz == int(case.padded.max())
    assert route(T, p4.max_nnz) == int(name != "complete")
    if name in ("k12", "row252"):
        assert p4.max_nnz > 256
    tx, tw, tb = up(x), up(w), up(b).reshape(-1)
    close(c_fwd(p4.desc(), tx, tw, tb), ref, atol=F.ATOL, rel=F.REL["fwd"], what="%s fwd, row-padded" % name)
    c4 = p4.compact4()
    assert (c4 is not None) == case.compact_ok
    if c4 is not None:
        assert c4.unit_values == (name == "directed_unit")
        close(c_fwd(c4.desc(), tx, tw, tb), ref, atol=F.ATOL, rel=F.REL["fwd"], what="%s fwd, compact" % name)


def test_captured_replays_equal_eager():
    T = T0
    adjs, x, w, b, _ = batch(T, True)
    csr = container(adjs)
    desc = descriptor(csr, "kipf", T)                  # (the compact copy is built here, outside the capture)
    assert route(T, csr.padded4().max_nnz) == 1
    tx, tw, tb = up(x), up(w), up(b).reshape(-1)
    eager = c_fwd(desc, tx, tw, tb)
    out = torch.zeros_like(tx)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c_fwd(desc, tx, tw, tb, out)                   # warm-up on the capturing stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c_fwd(desc, tx, tw, tb, out)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(eager)), "a captured replay differs from the eager launch"
