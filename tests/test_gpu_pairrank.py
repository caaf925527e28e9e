"""The ranking of all node pairs on the GPU (csrc/pairrank.hip, ops.pair_rank / ops.pair_rank_table, kgcn_amd.predscore) against
the numpy restatement of predscore.py (tests/predscore_oracle.py) and the fixture the reference produced
(tests/golden/g10_predscore.npz): exact cases bit for bit, a random case within the derivable fp32 bound, the whole pipeline,
and reproducibility."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import predscore_oracle as O  # noqa: E402
from gpu_helpers import to_device as _t  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "g10_predscore.npz")


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def run(h, w, cutoff):
    from kgcn_amd import ops
    s, r, c = ops.pair_rank(_t(h), None if w is None else _t(w), cutoff)
    return s.cpu().numpy(), r.cpu().numpy(), c.cpu().numpy()


def same_list(got, ref):
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[2].dtype == np.int32
    assert got[0].shape == ref[0].shape
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))


# ---- 1. exact cases: entries in quarters within [-2, 2] (w in halves): every product and every partial sum is an fp32 number
# (|sum| <= 200 * 8 in steps of 1 / 32), so the score does not depend on the summation order and ties are abundant ------------
@functools.lru_cache(maxsize=None)
def exact_case(n, d, with_w):
    rng = np.random.default_rng(1000 * n + 2 * d + with_w)
    h = (rng.integers(-8, 9, (n, d)) / 4.0).astype(np.float32)
    w = (rng.integers(-4, 5, d) / 2.0).astype(np.float32) if with_w else None
    m = O.pair_scores(h, w)
    m32 = m.astype(np.float32)
    assert np.array_equal(m32.astype(np.float64), m)
    full = O.sort_prediction_score(m32, 0)
    tied = np.nonzero(full[0][1:] == full[0][:-1])[0]
    # a cutoff whose last entry and the first one left out have one score (the middle one of those there are); none at N = 2
    cut = int(tied[len(tied) // 2]) + 1 if len(tied) else 1
    return h, w, full, cut


@pytest.mark.parametrize("cutoff", ["one", "tie", "all"])
@pytest.mark.parametrize("with_w", [0, 1])
@pytest.mark.parametrize("d", [1, 8, 33, 128, 200])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 130])
def test_exact_list_bit_for_bit(n, d, with_w, cutoff):
    h, w, full, cut = exact_case(n, d, with_w)
    total = n * (n - 1) // 2
    if n > 2:
        assert full[0][cut - 1] == full[0][cut]                       # the cutoff does cut through a tie group
    k = {"one": 1, "tie": cut, "all": 0}[cutoff]
    kk = k if k else total
    same_list(run(h, w, k), tuple(a[:kk] for a in full))
    if cutoff == "all":
        same_list(run(h, w, total), full)                             # cutoff = the pair count, and beyond it: all as well
        same_list(run(h, w, total + 5), full)


def test_all_zero_scores_are_one_tie_group():
    rng = np.random.default_rng(5)
    h = np.zeros((70, 5), np.float32)
    h[rng.random(h.shape) < 0.5] = -0.0
    assert np.signbit(h).any() and not np.signbit(h).all()
    full = O.sort_prediction_score(O.pair_scores(h).astype(np.float32), 0)
    assert not full[0].view(np.uint32).any()
    for k in (0, 100):
        same_list(run(h, None, k), tuple(a[:k or None] for a in full))
    w = np.full(5, -1.0, np.float32)                                  # the scaled operand flips every sign
    same_list(run(h, w, 0), full)


def test_nan_row_ranks_last():
    h, _, _, _ = exact_case(65, 8, 0)
    h = h.copy()
    h[h[:, 3] == 0, 3] = 0.25                                         # no inf * 0
    h[5] = np.nan
    h[64, 3] = np.inf                                                 # infinities are numbers: +inf first, -inf before the NaNs
    full = O.sort_prediction_score(O.pair_scores(h).astype(np.float32), 0)
    assert np.isnan(full[0][-64:]).all() and not np.isnan(full[0][:-64]).any()
    assert np.isposinf(full[0][0]) and np.isneginf(full[0][-65])
    same_list(run(h, None, 0), full)
    same_list(run(h, None, 2050), tuple(a[:2050] for a in full))       # a cutoff inside the NaN group


# ---- 2. random fp32 rows: properties against fp64 within the bound of an fp32 dot product ---------------------------------------
@pytest.mark.parametrize("with_w", [0, 1])
def test_random_rows_within_the_fp32_bound(with_w):
    """tol_ij = (D + 2) 2^-24 sum_k |h_ik w_k h_jk|: D roundings of the fma chain, one of the scaled operand, one to spare."""
    n, d, cutoff = 300, 128, 10000
    rng = np.random.default_rng(7 + with_w)
    h = rng.standard_normal((n, d)).astype(np.float32)
    w = rng.standard_normal(d).astype(np.float32) if with_w else None
    s, r, c = run(h, w, cutoff)
    ref, tol = O.pair_scores(h, w), (d + 2) * 2.0 ** -24 * O.pair_bounds(h, w)
    assert len(s) == cutoff and np.all(r < c) and np.all(r >= 0) and np.all(c < n)
    code = r.astype(np.int64) * n + c
    assert len(np.unique(code)) == cutoff
    s64 = s.astype(np.float64)
    later = (s64[1:] < s64[:-1]) | ((s64[1:] == s64[:-1]) & (code[1:] < code[:-1]))      # (score, row, col) descending
    assert later.all()
    worst = np.abs(s64 - ref[r, c]) / tol[r, c]
    print("max |score - fp64| / tol = %.3f" % worst.max())
    assert worst.max() <= 1.0
    left = np.ones((n, n), bool)
    left[np.tril_indices(n)] = False
    left[r, c] = False
    assert left.sum() == n * (n - 1) // 2 - cutoff
    over = (ref - tol)[left] - s64[-1]
    print("max over the smallest returned score among the omitted (beyond tol) = %.3e" % over.max())
    assert over.max() <= 0.0


# ---- 3. the whole pipeline on the reference's own table -------------------------------------------------------------------
def check_against(res, ref, score_bits):
    assert np.array_equal(_bits(res.score), score_bits)
    assert np.array_equal(res.row.cpu().numpy(), ref["row"]) and np.array_equal(res.col.cpu().numpy(), ref["col"])
    for name in ("score_ranking", "train_edge", "test_edge", "new_edge"):
        assert np.array_equal(getattr(res, name).cpu().numpy().astype(np.int64), np.asarray(ref[name], np.int64)), name
    for name in ("total", "total_wo_train", "total_target_edges", "total_train_edges", "total_test_edges"):
        assert getattr(res, name) == int(ref[name]), name
    for name in ("top_ratio", "test_edges_in_toplist", "enrichment"):
        assert list(getattr(res, name)) == np.asarray(ref[name]).tolist(), name


def test_pipeline_equals_the_reference_table(tmp_path):
    from kgcn_amd import predscore
    g = np.load(GOLDEN)
    res = predscore.rank_links(_t(g["h"]), g["label_list"], g["test_label_list"], cutoff=int(g["cutoff"]))
    check_against(res, g, g["score"].view(np.uint32))
    assert res.covered == [True] * 10 and len(res.lines()) == 15
    # a cutoff too small for the 10 % line (66 entries that are no train edge): the count is that of the shorter table
    ref = O.rank_links(g["h"], g["label_list"], g["test_label_list"], cutoff=50, matrix=O.pair_scores(g["h"]).astype(np.float32))
    small = predscore.rank_links(_t(g["h"]), g["label_list"], g["test_label_list"], cutoff=50)
    check_against(small, ref, ref["score"].view(np.uint32))
    assert small.covered == ref["covered"] and small.covered[0] and not small.covered[-1]
    # the files: header and columns of predscore.py:248-249, one line per entry; the label sets in sorted order
    predscore.write_score_table(res, str(tmp_path / "score.txt"), ["n%d" % i for i in range(40)])
    lines = open(str(tmp_path / "score.txt")).read().splitlines()
    assert lines[0].split("\t") == ["row", "col", "gene1", "gene2", "score", "score_ranking", "train_edge", "test_edge", "new_edge"]
    assert len(lines) == 301
    first = lines[1].split("\t")
    assert first[:4] == [str(g["row"][0]), str(g["col"][0]), "n%d" % g["row"][0], "n%d" % g["col"][0]]
    assert np.float32(first[4]) == g["score"][0] and first[5:] == ["1.0", str(g["train_edge"][0]), str(g["test_edge"][0]), str(g["new_edge"][0])]
    predscore.write_label_sets(res, str(tmp_path / "test.tsv"), str(tmp_path / "train.tsv"))
    test = [tuple(map(int, l.split("\t"))) for l in open(str(tmp_path / "test.tsv")).read().splitlines()]
    train = [tuple(map(int, l.split("\t"))) for l in open(str(tmp_path / "train.tsv")).read().splitlines()]
    assert test == O.label_pairs(g["test_label_list"]) and len(train) == 120
    assert sorted(test + train) == O.target_pairs(g["label_list"], g["test_label_list"])


def test_table_with_ties_against_the_oracle():
    """The fixture has no tied scores: score_ranking's shared ranks, empty code sets and thresholds beyond the list, on an exact
    list full of ties (several workgroups of entries)."""
    import torch
    from kgcn_amd import ops
    n = 63
    h, w, full, _ = exact_case(n, 1, 0)
    rng = np.random.default_rng(3)
    iu = np.stack(np.triu_indices(n, 1), 1)
    pick = iu[rng.permutation(len(iu))[:400]]
    target, test = sorted(map(tuple, pick.tolist())), sorted(map(tuple, pick[:90].tolist()))
    s, r, c = (torch.as_tensor(a, device="cuda") for a in (full[0][:1500], full[1][:1500], full[2][:1500]))
    tr, te, nw = O.convert(full[1][:1500], full[2][:1500], target, test)
    rank = O.score_ranking(full[0][:1500])
    assert len(np.unique(rank)) < 200                                  # ties share ranks
    top = [0, 1, 17, 256, 257, 1000, int((tr == 0).sum()), int((tr == 0).sum()) + 1, 5000]
    kept = te[tr == 0]
    out = ops.pair_rank_table(s, r, c, ops.pair_codes(target, "cuda"), ops.pair_codes(test, "cuda"), top)
    for got, ref in zip(out[:4], (tr, te, nw, rank)):
        assert np.array_equal(got.cpu().numpy().astype(np.int64), ref)
    assert out[4].tolist() == [int(kept[:t].sum()) for t in top]
    assert out[5].tolist() == [int(len(kept) >= t) for t in top]
    none = ops.pair_codes([], "cuda")
    out = ops.pair_rank_table(s, r, c, none, none, [10])
    assert not out[0].any() and not out[1].any() and out[2].all() and out[4].tolist() == [0] and out[5].tolist() == [1]


@pytest.mark.parametrize("variant", ["ip", "distmult"])
def test_model_rank_links(variant):
    import torch
    from kgcn_amd import models
    g = np.load(GOLDEN)
    model = models.LinkPredictionNet(variant, 40, num_relations=3, embedding_dim=8, device=torch.device("cuda"))
    with torch.no_grad():
        model.embedding.copy_(_t(g["h"]))
    w = None
    if variant == "distmult":
        w = (np.arange(8) - 3.0).astype(np.float32) / 2.0                                # halves: the scores stay exact
        with torch.no_grad():
            model.distmult.w[0][2].copy_(_t(w))
        with pytest.raises(ValueError):
            model.rank_links(None, g["label_list"], g["test_label_list"])
    res = model.rank_links(None, g["label_list"], g["test_label_list"], relation=2 if variant == "distmult" else None, cutoff=300)
    ref = O.rank_links(g["h"], g["label_list"], g["test_label_list"], w=w, cutoff=300, matrix=O.pair_scores(g["h"], w).astype(np.float32))
    check_against(res, ref, ref["score"].view(np.uint32))


# ---- 4. reproducibility ------------------------------------------------------------------------------------------------
def test_same_call_twice_gives_the_same_bytes():
    rng = np.random.default_rng(11)
    h = rng.standard_normal((130, 128)).astype(np.float32)
    w = rng.standard_normal(128).astype(np.float32)
    a, b = run(h, w, 3000), run(h, w, 3000)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    a, b = run(h, None, 0), run(h, None, 0)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
