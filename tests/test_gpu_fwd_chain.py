"""The aggregator wave of the FULL-shape pairs forward (graphconv_fwd_full_kernel, aggregate_rows_full4) against the one-wave kernel.

The pairs forward reads the slot words and the first column words of all 32 rows of a graph up front, keeps all eight aggregation
passes in flight and, in the first two passes, gathers a long row's SECOND group beside its first one (dropped by a select where
the row has none).  Every sum must still be the one graphconv_fwd_wave_kernel computes, bit for bit.  Every case here runs T = 16,384 (every pair whole) or 16,385
(short pairs) graphs through the pairs kernel in one launch and through the one-wave kernel in slices below its threshold, on
hand-made 32-node graphs tiled over the batch:

  len0_15, len16_32   every row length 0..32 (a compact slot holds a row's first group at most 127 groups into its graph, so the
                      33 lengths take two graphs; len1_32 carries 1..32 in ONE graph in the row-padded layout)
  bounds              row lengths 4, 5, 8, 9 (the group boundaries)
  dense12 / 8 / 5     second groups in every pass; dense12 a third group as well.  (The complete graph K32 has 1,024 entries: two
                      slices of it do not fit the pairs kernel's LDS and it takes the one-wave route, tests/test_gpu_fwd_pairs.py;
                      dense24, 768 entries, is the densest that fits, row-padded layout only.)
  star0, star31       one 32-entry row, the rest one entry
  empty, sparse3      no entries at all; three non-empty rows
  ties3, ties4        equal-length rows (slot ties)
  half17              17 rows of 5 entries, 15 of 2: the fifth pass has ONE row with a second group
  one9                one row of 9 entries, the rest 3
  rnd*                random directed graphs, rows of 0..12 entries

The row-padded layout keeps aggregate_rows_full2 in the pairs kernel; it runs the same cases plus len1_32 and dense24.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, D = 32, 64
T0 = 16384                      # fused.hip: KGCN_FWD_PAIRS_MIN_GRAPHS
SLICE = 6000                    # graphs per launch of the one-wave kernel
COMPACT = 0x104
GUARD = 4096                    # floats in front of and behind the output
FILL = 0x7fc0a5a5               # a quiet NaN with a payload no kernel produces


def dev():
    return torch.device("cuda:0")


def _rows(lengths, rng):
    """a graph with lengths[r] entries in row r, distinct random columns per row"""
    r = np.repeat(np.arange(N), lengths)
    c = np.concatenate([rng.permutation(N)[:k] for k in lengths] + [np.zeros(0, np.int64)])
    return r.astype(np.int64), c.astype(np.int64)


def _star(centre):
    others = np.array([i for i in range(N) if i != centre])
    r = np.concatenate([np.full(N, centre), others])
    c = np.concatenate([np.arange(N), np.full(N - 1, centre)])
    return r.astype(np.int64), c.astype(np.int64)


@functools.lru_cache(maxsize=None)
def patterns(extra):
    """[(name, row, col)]: the hand-made graphs; extra: the two that only the row-padded layout holds"""
    rng = np.random.default_rng(50_051)
    L = lambda a: np.asarray(a, np.int64)
    out = [("len0_15", *_rows(L(list(range(16)) * 2), rng)),
           ("len16_32", *_rows(L([0] * 7 + list(range(16, 33)) + [0] * 8), rng)),
           ("bounds", *_rows(L([4, 5, 8, 9] * 8), rng)),
           ("dense12", *_rows(L([12] * N), rng)),
           ("dense8", *_rows(L([8] * N), rng)),
           ("dense5", *_rows(L([5] * N), rng)),
           ("star0", *_star(0)),
           ("star31", *_star(31)),
           ("empty", L([]), L([])),
           ("sparse3", *_rows(L([0] * 5 + [7] + [0] * 12 + [1] + [0] * 12 + [4]), rng)),
           ("ties3", *_rows(L([3] * N), rng)),
           ("ties4", *_rows(L([4] * N), rng)),
           ("half17", *_rows(rng.permutation(L([5] * 17 + [2] * 15)), rng)),
           ("one9", *_rows(L([3] * 20 + [9] + [3] * 11), rng))]
    for i in range(12):
        out.append(("rnd%d" % i, *_rows(rng.integers(0, 13, size=N), rng)))
    if extra:
        out.append(("len1_32", *_rows(rng.permutation(np.arange(1, 33)), rng)))
        out.append(("dense24", *_rows(L([24] * N), rng)))
    for _, r, c in out:
        r.setflags(write=False)
        c.setflags(write=False)
    return tuple(out)


def test_patterns_cover_what_they_name():
    pats = {name: np.bincount(r, minlength=N) for name, r, _ in patterns(True)}
    assert len(patterns(False)) == 26
    assert sorted(set(pats["len0_15"]) | set(pats["len16_32"])) == list(range(33))
    assert sorted(pats["len1_32"]) == list(range(1, 33))
    assert set(pats["bounds"]) == {4, 5, 8, 9}
    assert sorted(pats["star0"])[-2:] == [1, 32] and pats["star31"][31] == 32
    assert pats["empty"].sum() == 0 and (pats["sparse3"] > 0).sum() == 3
    assert (np.sort(pats["half17"])[::-1][16] == 5) and (np.sort(pats["half17"])[::-1][17] == 2)
    for name, r, c in patterns(True):
        assert len(set(zip(r.tolist(), c.tolist()))) == r.shape[0], name      # no entry twice


def arrays(lo, hi, extra, unit):
    """graphs lo..hi-1 of the tiled batch (graph t is pattern t mod P) as triples; the values depend on the entry alone"""
    pats = patterns(extra)
    P = len(pats)
    gs, rs, cs, vs = [], [], [], []
    for k, (_, r, c) in enumerate(pats):
        ts = np.arange(lo + (k - lo) % P, hi, P)
        if r.shape[0] == 0 or ts.shape[0] == 0:
            continue
        v = np.ones(r.shape[0], np.float32) if unit else np.random.default_rng(k).uniform(-1.5, 1.5, r.shape[0]).astype(np.float32)
        gs.append(np.repeat(ts - lo, r.shape[0])); rs.append(np.tile(r, ts.shape[0])); cs.append(np.tile(c, ts.shape[0]))
        vs.append(np.tile(v, ts.shape[0]))
    return np.concatenate(gs).astype(np.int64), np.concatenate(rs), np.concatenate(cs), np.concatenate(vs)


def descriptor(csr, layout, T):
    from kgcn_amd import ops
    if layout == "pad4":
        return csr.padded4().desc()
    desc = ops._fused_adjacency(csr, False, T, D, D, False)
    assert desc.row_pad == COMPACT
    c4 = csr.padded4().compact4()
    assert c4 is not None and c4.unit_values == (layout == "unit")
    return desc


def route(T, max_nnz):
    from kgcn_amd._lib import lib
    return lib.kgcn_graphconv_fwd_pairs_route(T, N, D, D, max_nnz)


def c_fwd(desc, x, w, b, out):
    from kgcn_amd._lib import check, current_stream, lib, ptr
    check(lib.kgcn_graphconv_fwd_f32(desc, ptr(x), ptr(w), ptr(b), D, D, ptr(out), current_stream()), "kgcn_graphconv_fwd_f32")
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


def operands(T, seed):
    gen = torch.Generator(device=dev())
    gen.manual_seed(seed)
    x = torch.randn((T, N, D), device=dev(), generator=gen)
    w = (torch.rand((D, D), device=dev(), generator=gen) - 0.5) * 0.6
    b = torch.randn((D,), device=dev(), generator=gen)
    return x, w, b


def pairs_launch(T, layout, extra, x, w, b):
    """(out of the pairs kernel, the buffer that holds it between guard words)"""
    from kgcn_amd import BatchedCSR
    csr = BatchedCSR.from_arrays(*arrays(0, T, extra, layout == "unit"), T, N, N, device=dev())
    assert route(T, csr.padded4().max_nnz) == 1, "the batch does not take the pairs kernel"
    desc = descriptor(csr, layout, T)
    bufs = []
    for _ in range(2):                                       # twice: the same words both times, guards included
        buf = torch.full((GUARD + T * N * D + GUARD,), FILL, dtype=torch.int32, device=dev())
        out = buf[GUARD:GUARD + T * N * D].view(torch.float32).view(T, N, D)
        assert out.data_ptr() % 16 == 0
        c_fwd(desc, x, w, b, out)
        torch.cuda.synchronize()
        bufs.append(buf)
    assert torch.equal(bufs[0], bufs[1]), "the output (or a guard word) differs between two launches on the same operands"
    return out, buf


def one_wave(T, layout, extra, x, w, b):
    """the same batch through the one-wave kernel, in slices below the pairs threshold"""
    from kgcn_amd import BatchedCSR
    ref = torch.full((T, N, D), float("nan"), device=dev())
    for s in range(0, T, SLICE):
        e = min(T, s + SLICE)
        part = BatchedCSR.from_arrays(*arrays(s, e, extra, layout == "unit"), e - s, N, N, device=dev())
        assert route(e - s, part.padded4().max_nnz) == 0
        piece = torch.empty((e - s, N, D), device=dev())
        c_fwd(descriptor(part, layout, e - s), x[s:e].contiguous(), w, b, piece)
        ref[s:e] = piece
    torch.cuda.synchronize()
    return ref


def both_kernels(T, layout, extra, x, w, b):
    out, buf = pairs_launch(T, layout, extra, x, w, b)
    return out, buf, one_wave(T, layout, extra, x, w, b)


def check_guards(buf, T):
    front, back = buf[:GUARD], buf[GUARD + T * N * D:]
    assert int((front != FILL).sum()) == 0, "%d words in front of the output were written" % int((front != FILL).sum())
    assert int((back != FILL).sum()) == 0, "%d words behind the output were written" % int((back != FILL).sum())
    left = buf[GUARD:GUARD + T * N * D] == FILL
    assert int(left.sum()) == 0, "%d elements of the output were not written (first at flat index %d)" % (
        int(left.sum()), int(torch.nonzero(left)[0]))


def first_difference(out, ref, extra):
    bad = torch.nonzero((bits(out) != bits(ref)).flatten())
    if bad.numel() == 0:
        return None
    t, r, c = np.unravel_index(int(bad[0]), (out.shape[0], N, D))
    return "%d elements differ; first: graph %d (%s) row %d column %d: %r against %r" % (
        bad.numel(), t, patterns(extra)[t % len(patterns(extra))][0], r, c, float(out[t, r, c]), float(ref[t, r, c]))


@pytest.mark.parametrize("layout,extra", [("unit", False), ("values", False), ("pad4", False), ("pad4", True)])
@pytest.mark.parametrize("T", [T0, T0 + 1])
def test_bit_equal_to_the_one_wave_kernel(T, layout, extra):
    x, w, b = operands(T, 7 * T + len(layout))
    out, buf, ref = both_kernels(T, layout, extra, x, w, b)
    check_guards(buf, T)
    assert bool(torch.isfinite(ref).all())
    assert first_difference(out, ref, extra) is None, first_difference(out, ref, extra)


@pytest.mark.parametrize("layout", ["unit", "values"])
def test_non_finite_rows_stay_with_their_neighbours(layout):
    """+inf, -inf and NaN in single rows of x: a row of the output that has none of those nodes as a neighbour is finite and equal
    to the one-wave kernel's, whatever the gathers beside its own groups read"""
    T = T0 + 1
    x, w, b = operands(T, 99)
    P = len(patterns(False))
    poison = {3: float("inf"), 17: float("-inf"), 30: float("nan")}
    for node, v in poison.items():
        x[:, node, :] = v
    out, buf, ref = both_kernels(T, layout, False, x, w, b)
    check_guards(buf, T)
    clean = torch.ones((P, N), dtype=torch.bool)
    for k, (_, r, c) in enumerate(patterns(False)):
        hit = np.isin(c, list(poison))
        clean[k, np.unique(r[hit])] = False
    assert int(clean.sum()) > P * N // 4 and int((~clean).sum()) > P * N // 8
    mask = clean.repeat((T + P - 1) // P, 1)[:T].to(dev())
    assert bool(torch.isfinite(out[mask]).all()), "a row without a non-finite neighbour came out non-finite"
    assert bool(torch.isfinite(ref[mask]).all())
    assert torch.equal(bits(out[mask]), bits(ref[mask]))
    assert not bool(torch.isfinite(out[~mask]).any()), "a row WITH a non-finite neighbour came out finite"
    assert torch.equal(torch.isnan(out), torch.isnan(ref))


@pytest.mark.parametrize("layout", ["unit", "values"])
def test_signed_zeros(layout):
    """x = 0 and a bias of -0.0: every sum is a sum of zeros, whose sign an extra +0 term would change"""
    T = T0 + 1
    _, w, _ = operands(T, 5)
    x = torch.zeros((T, N, D), device=dev())
    b = torch.full((D,), -0.0, device=dev())
    assert int(bits(b)[0]) == -2 ** 31
    out, buf, ref = both_kernels(T, layout, False, x, w, b)
    check_guards(buf, T)
    assert bool((out == 0).all())
    assert first_difference(out, ref, False) is None, first_difference(out, ref, False)
    x = torch.full((T, N, D), -0.0, device=dev())           # and with x = -0: products of both signs
    out, buf, ref = both_kernels(T, layout, False, x, w, b)
    print("negative zeros in the one-wave kernel's output: %d of %d" % (int((bits(ref) != 0).sum()), ref.numel()))
    assert bool((out == 0).all())
    assert first_difference(out, ref, False) is None, first_difference(out, ref, False)
