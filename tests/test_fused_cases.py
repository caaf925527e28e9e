"""CPU checks of tests/fused_cases.py, the batches tests/test_gpu_fused_cases.py runs on the device: every case sits on the edge it
names (exact row-padded entry counts, A != A^T, what the compact slot can hold), the dense adjacency is the accumulated triples, a
seed reproduces its batch -- and the written tolerances are wide enough for correct float32 arithmetic at these densities, judged on
a plain numpy float32 restatement of the formulas, never on a kernel.  Every test prints its figures (pytest -s / -rP)."""
import numpy as np
import pytest

import fused_cases as F

ALL = F.FULL_CASES + F.PACK_CASES
T_SMALL = {"pack2": 65, "pack4": 67}


def small(name):
    return F.build(name, T_SMALL.get(name, 5))


def live(case):
    return np.flatnonzero(np.bincount(case.graph, minlength=case.T))


@pytest.mark.parametrize("name", ALL + ["row256"])
def test_dense_is_the_accumulated_triples_and_seed_reproduces(name):
    c = small(name)
    dense = np.zeros((c.T, c.N, c.N))
    for g, r, col, v in zip(c.graph, c.row, c.col, c.val):               # one entry after the other: duplicates accumulate
        dense[g, r, col] += float(v)
    assert np.array_equal(dense, c.dense)
    F._build.cache_clear()
    again = small(name)
    assert again is not c
    for a, b in zip(c[5:12], again[5:12]):
        assert np.array_equal(a, b)
    assert (c.compact_ok, c.compact_ok_t) == (again.compact_ok, again.compact_ok_t)
    other = F.build(name, c.T, F.SEEDS.get(name, 0) + 1)
    assert other.val.shape != c.val.shape or not np.array_equal(other.val, c.val)
    # unsorted: neither the graphs nor the rows inside a graph come in order
    assert np.any(np.diff(c.graph) < 0) and np.any(np.diff((c.graph * c.N + c.row)[np.argsort(c.graph, kind="stable")]) < 0)
    # the copies of a duplicated entry share their sign: |A| is the accumulated |values|
    absd = np.zeros_like(dense)
    np.add.at(absd, (c.graph, c.row, c.col), np.abs(c.val.astype(np.float64)))
    assert np.array_equal(absd, np.abs(c.dense))


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("big", [False, True])
def test_empty_ends_asymmetry_and_values(name, big):
    c = F.build(name, 2049) if (big and name in F.FULL_CASES) else small(name)
    cnt = np.bincount(c.graph, minlength=c.T)
    assert cnt[0] == 0 and cnt[-1] == 0 and np.all(cnt[1:-1] > 0)
    for t in live(c):
        assert not np.array_equal(c.dense[t], c.dense[t].T), (name, t)
    if name == "directed_unit":
        assert np.all(c.val == 1.0) and c.dense.max() == 2.0 and np.all(np.isin(c.dense, (0.0, 1.0, 2.0)))
    else:
        assert np.all((np.abs(c.val) >= np.float32(0.2)) & (np.abs(c.val) <= np.float32(0.8)))
        assert (c.val < 0).any() and (c.val > 0).any()


@pytest.mark.parametrize("T", [5, 2049])
def test_directed_cases(T):
    d, u = F.build("directed", T), F.build("directed_unit", T)
    assert all(np.array_equal(a, b) for a, b in zip((d.graph, d.row, d.col), (u.graph, u.row, u.col)))       # the same patterns
    stored = np.zeros((T, 32, 32), bool)
    stored[d.graph, d.row, d.col] = True
    assert not (stored & stored.transpose(0, 2, 1)).any()                 # an entry's reverse (and a self loop) is never stored
    _, _, rows = F.padded_counts(d.graph, d.row, T, 32)
    per = np.bincount(d.graph, minlength=T)[1:-1]
    assert per.min() >= 30 and per.max() <= 60
    assert np.all(rows[1:-1].max(axis=1) == 20) and np.all((rows[1:-1] == 0).sum(axis=1) >= 6)
    dup = per - stored.sum(axis=(1, 2))[1:-1]
    assert np.all(dup == 9)                                               # three doubled entries and six in the long row
    assert u.dense[1:-1].max(axis=(1, 2)).min() == 2.0                    # every graph holds duplicates
    assert d.padded.max() <= 220 and d.padded_t.max() <= 220
    assert d.compact_ok and d.compact_ok_t and u.compact_ok and u.compact_ok_t
    print("directed T=%d: entries %d..%d, row-padded A %d..%d, A^T %d..%d" % (T, per.min(), per.max(), d.padded[1:-1].min(),
                                                                             d.padded.max(), d.padded_t[1:-1].min(), d.padded_t.max()))


@pytest.mark.parametrize("T", [5, 2049])
@pytest.mark.parametrize("edge", [220, 224])
def test_edge_cases(edge, T):
    c = F.build("edge%d" % edge, T)
    for pad in (c.padded, c.padded_t):                                    # the backward reads A^T: the edge holds there too
        assert pad[1] == edge and np.all(np.delete(pad, 1) < 220)
    _, _, rows = F.padded_counts(c.graph, c.row, T, 32)
    _, _, cols = F.padded_counts(c.graph, c.col, T, 32)
    assert rows.max() <= 60 and cols.max() <= 60
    assert c.compact_ok and c.compact_ok_t
    # the arithmetic of bwd_full_route (fused.hip): 8736 + 16 max_nnz <= 12288 holds at 220 and fails at 224
    assert (8736 + 16 * int(c.padded_t.max()) <= 12288) == (edge == 220)


def test_dense_and_long_row_cases():
    for T in (5, 2049):
        k12, full, r64, r252 = (F.build(n, T) for n in ("k12", "complete", "row64", "row252"))
        _, _, rows = F.padded_counts(k12.graph, k12.row, T, 32)
        stored = np.zeros((T, 32, 32), bool)
        stored[k12.graph, k12.row, k12.col] = True
        assert np.all(rows[1:-1] == 12) and np.all(stored.sum(axis=2)[1:-1] == 12) and np.all(stored.sum(axis=1)[1:-1] == 12)
        assert np.all(k12.padded[1:-1] == 384) and np.all(k12.padded_t[1:-1] == 384) and k12.compact_ok and k12.compact_ok_t
        assert np.all(full.padded[1:-1] == 1024) and np.all(full.padded_t[1:-1] == 1024)
        assert not full.compact_ok and not full.compact_ok_t             # rows start beyond entry 508
        assert np.all(np.bincount(full.graph, minlength=T)[1:-1] == 1024) and np.all(full.dense[1:-1] != 0)
        _, _, rows = F.padded_counts(r64.graph, r64.row, T, 32)
        _, _, cols = F.padded_counts(r64.graph, r64.col, T, 32)
        assert np.all(rows[1:-1].max(axis=1) == 64) and np.all(cols[1:-1].max(axis=1) == 64)
        assert r64.padded.max() <= 220 and r64.padded_t.max() <= 220
        assert not r64.compact_ok and not r64.compact_ok_t               # a row (of A and of A^T) longer than 60 entries
        assert np.all((rows[1:-1] == 0).sum(axis=1) >= 3)
        _, _, rows = F.padded_counts(r252.graph, r252.row, T, 32)
        srt = np.sort(rows[1:-1], axis=1)
        assert np.all(srt[:, -1] == 252) and np.all(srt[:, -2] <= 4)
        assert np.all(r252.padded[1:-1] == 376) and not r252.compact_ok
        assert r252.padded_t.max() > 220                                  # the backward of this case is the generic kernel's
    r256 = F.build("row256", 5)
    _, _, rows = F.padded_counts(r256.graph, r256.row, 5, 32)
    assert np.all(rows[1:-1].max(axis=1) == 256)


def test_pack_cases():
    p2, p4 = F.build("pack2", 65), F.build("pack4", 67)
    assert (p2.N, p2.din, p2.dout, p4.N, p4.din, p4.dout) == (16, 12, 36, 8, 5, 6)
    for c, per in ((p2, 192), (p4, 96)):
        _, _, rows = F.padded_counts(c.graph, c.row, c.T, c.N)
        _, _, cols = F.padded_counts(c.graph, c.col, c.T, c.N)
        assert np.all(rows[1:-1] == 12) and np.all(cols[1:-1] == 12)
        assert np.all(c.padded[1:-1] == per) and np.all(c.padded_t[1:-1] == per)
        assert c.padded[0] == 4 * c.N
    stored = np.zeros((65, 16, 16), bool)
    stored[p2.graph, p2.row, p2.col] = True
    assert np.all(stored.sum(axis=2)[1:-1] == 12)                         # pack2: 12 DISTINCT columns
    assert np.all(p4.dense[1:-1] != 0)                                    # pack4: all 8 columns, 4 of them twice
    # graphs per tile: a pack holds 384 > 256 entries, in the middle of the batch
    assert p2.padded[2:4].sum() == 384 and p4.padded[4:8].sum() == 384
    assert F.build("pack2", 67).T % 2 == 1 and p4.T % 4 == 3


def test_stream_T_reads_the_constant():
    T = F.stream_T()
    assert T == 10923                                                     # (256 << 20) / (32 * 64 * 4 * 3) = 10922.67
    assert T * 32 * 64 * 4 * 3 > (256 << 20) >= (T - 1) * 32 * 64 * 4 * 3


# ---- the tolerances: judged on the float32 restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("name,T", F.gpu_runs())
def test_written_tolerances_leave_room_for_float32(name, T):
    """For every quantity the GPU test holds to atol + rel * max|ref|, correct float32 arithmetic (restate_f32) stays under a quarter
    of it; the others are listed in F.COMPONENTWISE with the restatement's largest err / (2^-24 S), which holds here as a bound."""
    ref = F.reference(name, T)
    got = dict(zip(("fwd", "dx", "dw", "db"), F.restate_f32(name, T)))
    scale = {"dw": ref.s_dw, "db": ref.s_db}
    for what in ("fwd", "dx", "dw", "db"):
        r = getattr(ref, what)
        err = np.abs(got[what].astype(np.float64) - r)
        share = float(err.max()) / F.written_tol(what, r)
        comp = F.COMPONENTWISE.get((name, T, what))
        if comp is None:
            print("%s T=%d %s: float32 restatement at %.2f of the written tolerance %.3e" % (name, T, what, share, F.written_tol(what, r)))
            assert share < 0.25, (name, T, what, share)
        else:
            ratio = float((err / (F.EPS * scale[what].reshape(err.shape))).max())
            print("%s T=%d %s: float32 restatement at %.2f of the written tolerance: componentwise, err / (2^-24 S) = %.2f "
                  "(recorded %.2f, c = %.1f)" % (name, T, what, share, ratio, comp, 4 * comp))
            assert what in ("dw", "db") and share >= 0.25, "the written form serves here: drop the entry"
            assert ratio <= comp, (name, T, what, ratio, comp)
