"""CPU checks of the link ranking (run_enrichment.sh): the numpy restatement of predscore.py (tests/predscore_oracle.py) against
the fixture the reference itself produced (tests/golden/g10_predscore.npz, make_golden_predscore.py), the host logic of
kgcn_amd.predscore (label pairs, the top_ratio rounding), and the argument validation of the new entry points (no launch)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import predscore_oracle as O  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "g10_predscore.npz")
COLUMNS = ("row", "col", "score_ranking", "train_edge", "test_edge", "new_edge")
COUNTS = ("total", "total_wo_train", "total_target_edges", "total_train_edges", "total_test_edges")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def test_fixture_is_what_the_generator_promises(gold):
    h = gold["h"]
    assert h.shape == (40, 8) and h.dtype == np.float32
    k = h.astype(np.float64) * 64
    assert np.array_equal(k, np.round(k)) and np.abs(k).max() <= 64
    m = O.pair_scores(h)
    assert np.array_equal(m.astype(np.float32).astype(np.float64), m)                     # H H^T is exact in fp32
    assert len(np.unique(m[np.triu_indices(40, 1)])) == 780                               # no ties
    for name in ("label_list", "test_label_list"):
        ll = gold[name][0]
        assert np.any(ll[:, 0] > ll[:, 2]) and np.any(ll[:, 0] < ll[:, 2])                # both storage orders
        assert len(O.label_pairs(gold[name])) < len(ll)                                   # repeated rows
    assert int(gold["cutoff"]) == 300 == len(gold["row"])


def test_oracle_reproduces_the_reference_table(gold):
    """Every column and every printed count of predscore.py on the fixture."""
    m32 = O.pair_scores(gold["h"]).astype(np.float32)
    out = O.rank_links(gold["h"], gold["label_list"], gold["test_label_list"], cutoff=int(gold["cutoff"]), matrix=m32)
    assert out["score"].dtype == np.float32
    assert np.array_equal(out["score"].view(np.uint32), gold["score"].view(np.uint32))
    for name in COLUMNS:
        assert np.array_equal(out[name], gold[name]), name
    for name in COUNTS:
        assert out[name] == int(gold[name]), name
    assert out["top_ratio"] == gold["top_ratio"].tolist()
    assert out["test_edges_in_toplist"] == gold["test_edges_in_toplist"].tolist()
    assert out["enrichment"] == gold["enrichment"].tolist()
    assert all(out["covered"])
    assert len(O.label_pairs(gold["test_label_list"])) == 30 and len(O.target_pairs(gold["label_list"], gold["test_label_list"])) == 150


def test_oracle_order_ties_zeros_and_nan():
    m = np.zeros((4, 4), np.float32)
    m[0, 1], m[0, 2], m[0, 3], m[1, 2], m[1, 3], m[2, 3] = 1.0, -0.0, 0.0, np.nan, 1.0, -np.inf
    s, r, c = O.sort_prediction_score(m, 0)
    assert list(zip(r.tolist(), c.tolist())) == [(1, 3), (0, 1), (0, 3), (0, 2), (2, 3), (1, 2)]
    assert s.view(np.uint32).tolist() == [0x3f800000, 0x3f800000, 0, 0, 0xff800000, 0x7fc00000]
    assert O.score_ranking(np.array([3.0, 2.0, 2.0, 1.0])).tolist() == [1, 2, 2, 4]
    assert O.sort_prediction_score(m, 2)[1].tolist() == [1, 0]


def test_label_pairs_host_logic(gold):
    from kgcn_amd import predscore
    ll = np.array([[[5, 2, 3, 5, 0, 9], [3, 2, 5, 3, 0, 1], [1, 2, 4, 1, 0, 0], [4, 2, 1, 4, 0, 2], [0, 2, 7, 0, 0, 3]]])
    assert predscore.label_pairs(ll).tolist() == [[0, 7], [1, 4], [3, 5]]
    assert predscore.label_pairs(ll[0]).tolist() == [[0, 7], [1, 4], [3, 5]]
    assert predscore.label_pairs(np.zeros((1, 0, 6), np.int32)).shape == (0, 2)
    for name in ("label_list", "test_label_list"):
        assert [tuple(p) for p in predscore.label_pairs(gold[name]).tolist()] == O.label_pairs(gold[name])
    with pytest.raises(ValueError):
        predscore.label_pairs(np.zeros((3, 2)))


def test_top_ratio_is_pythons_round_of_the_float_product(gold):
    from kgcn_amd import predscore
    assert predscore.top_ratios(int(gold["total_wo_train"])) == gold["top_ratio"].tolist()
    assert predscore.top_ratios(50, (1.0,)) == [0]                    # round(0.5): to even, not up
    assert predscore.top_ratios(150, (1.0,)) == [2]                   # round(1.5)
    assert predscore.top_ratios(250, (1.0,)) == [2]                   # round(2.5)
    assert predscore.top_ratios(350, (1.0,)) == [4]                   # 3.5
    # the ratio is p * 0.01 in floating point (7 * 0.01 = 0.07000000000000001), then the product, then round
    for total in (50, 650, 12497500, 12487520):
        assert predscore.top_ratios(total) == [round(total * (p * 0.01)) for p in predscore.TOP_PERCENT]
    assert predscore.TOP_PERCENT == tuple(float(p) for p in range(1, 11))


def test_pair_rank_validation_without_a_launch():
    from kgcn_amd import _lib
    lib = _lib.lib
    P = ctypes.c_void_p(4096)                                         # a non-NULL pointer nothing dereferences before the checks fail
    assert lib.kgcn_pair_rank_workspace_bytes(5000, 128, 0, 0) > 0
    assert lib.kgcn_pair_rank_workspace_bytes(5000, 128, 1500000, 0) >= 2 * 8 * 1500000
    assert lib.kgcn_pair_rank_workspace_bytes(5000, 128, 0, 1500000) >= 2 * 4 * 1500000
    assert lib.kgcn_pair_rank_workspace_bytes(65536, 256, 0, 0) > 0
    for n, d, cap, ent in ((1, 8, 0, 0), (65537, 8, 0, 0), (10, 0, 0, 0), (10, 257, 0, 0), (10, 8, -1, 0), (10, 8, (1 << 28) + 1, 0),
                           (10, 8, 0, -1), (10, 8, 0, (1 << 28) + 1)):
        assert lib.kgcn_pair_rank_workspace_bytes(n, d, cap, ent) == -1, (n, d, cap, ent)
    for n, d, cut, what in ((1, 8, 5, b"nodes"), (65537, 8, 5, b"nodes"), (10, 0, 5, b"dim"), (10, 257, 5, b"dim"),
                            (10, 8, -1, b"cutoff")):
        assert lib.kgcn_pair_rank_select_f32(P, n, d, None, cut, P, P, 1 << 20, None) != 0
        assert what in lib.kgcn_last_error(), (what, lib.kgcn_last_error())
        assert lib.kgcn_pair_rank_emit_f32(P, n, d, None, cut, P, 45, P, P, P, P, 1 << 20, None) != 0
        assert what in lib.kgcn_last_error(), (what, lib.kgcn_last_error())
    assert lib.kgcn_pair_rank_select_f32(None, 10, 8, None, 5, P, P, 1 << 20, None) != 0 and b"NULL" in lib.kgcn_last_error()
    assert lib.kgcn_pair_rank_select_f32(P, 10, 8, None, 5, None, P, 1 << 20, None) != 0 and b"NULL" in lib.kgcn_last_error()
    assert lib.kgcn_pair_rank_select_f32(P, 10, 8, None, 5, P, None, 1 << 20, None) != 0 and b"workspace" in lib.kgcn_last_error()
    assert lib.kgcn_pair_rank_select_f32(P, 10, 8, None, 5, P, P, 16, None) != 0 and b"workspace" in lib.kgcn_last_error()
    assert lib.kgcn_pair_rank_emit_f32(P, 10, 8, None, 5, P, 45, None, P, P, P, 1 << 20, None) != 0 and b"NULL" in lib.kgcn_last_error()
    assert lib.kgcn_pair_rank_emit_f32(P, 10, 8, None, 5, P, 4, P, P, P, P, 1 << 20, None) != 0 and b"capacity" in lib.kgcn_last_error()
    assert lib.kgcn_pair_rank_emit_f32(P, 10, 8, None, 0, P, 44, P, P, P, P, 1 << 20, None) != 0 and b"capacity" in lib.kgcn_last_error()
    assert lib.kgcn_pair_rank_emit_f32(P, 10, 8, None, 5, P, 45, P, P, P, P, 16, None) != 0 and b"workspace" in lib.kgcn_last_error()
    top = (ctypes.c_int64 * 17)(*range(17))

    def table(entries=10, nt=3, ns=2, ntop=10, score=P, target=P, hits=P, ws=P, wsb=1 << 20):
        return lib.kgcn_pair_rank_table_i32(score, P, P, entries, target, nt, P, ns, top, ntop, P, P, P, P, hits, P, ws, wsb, None)

    assert table(entries=0) != 0 and b"entries" in lib.kgcn_last_error()
    assert table(entries=(1 << 28) + 1) != 0 and b"entries" in lib.kgcn_last_error()
    assert table(nt=-1) != 0 and table(ns=-1) != 0
    assert table(ntop=17) != 0 and b"thresholds" in lib.kgcn_last_error()
    assert table(score=None) != 0 and b"NULL" in lib.kgcn_last_error()
    assert table(target=None) != 0 and b"NULL" in lib.kgcn_last_error()
    assert table(hits=None) != 0 and b"NULL" in lib.kgcn_last_error()
    assert table(ws=None) != 0 and b"workspace" in lib.kgcn_last_error()
    assert table(wsb=16) != 0 and b"workspace" in lib.kgcn_last_error()


def test_wrappers_refuse_host_tensors_and_bad_shapes():
    import torch
    from kgcn_amd import _lib, ops
    with pytest.raises(_lib.KgcnHipError):
        ops.pair_rank(torch.zeros((4, 3)))                            # a CPU tensor: there is no CPU path
    with pytest.raises(ValueError):
        ops.pair_codes([[3, 1]], "cpu")                               # row >= col
    with pytest.raises(ValueError):
        ops.pair_codes([[0, 65536]], "cpu")
    codes = ops.pair_codes([[1, 2], [0, 65535], [1, 2], [0, 1]], "cpu").numpy().view(np.uint32)
    assert codes.tolist() == [1, 65535, (1 << 16) | 2]
