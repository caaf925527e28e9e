"""The numpy oracle of the classical graph kernels (tests/graph_kernel_oracle.py) against the Grams the reference's own
weisfeiler_lehman_subtree_kernel / shortest_path_kernel produced (tests/golden/g13_graph_kernel.npz), and the host parts of
kgcn_amd/graph_kernel.py: the label ranks, dataset_graphs and the nested cross-validation.  No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import graph_kernel_oracle as O  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "g13_graph_kernel.npz")


@pytest.fixture(scope="module")
def z():
    return np.load(GOLDEN, allow_pickle=False)


@pytest.mark.parametrize("labels", ["node", "degree"])
@pytest.mark.parametrize("kind", ["wl", "sp"])
@pytest.mark.parametrize("prefix", ["small_", "two_"])
def test_oracle_equals_the_reference_grams(z, prefix, kind, labels):
    graphs = O.unpack_graphs(z, prefix)
    mine = O.wl_gram(graphs, 3, labels) if kind == "wl" else O.sp_gram(graphs, labels)
    assert mine.dtype == np.int64
    np.testing.assert_array_equal(mine, z["%s%s_%s" % (prefix, kind, labels)])
    norm, ref = O.normalize(mine), z["%s%s_%s_norm" % (prefix, kind, labels)]
    np.testing.assert_array_equal(norm.view(np.uint64), ref.view(np.uint64))


def test_small_set_holds_the_edge_cases(z):
    graphs = O.unpack_graphs(z, "small_")
    assert len(graphs) == 41 and max(g[0] for g in graphs) == 13
    sizes = [g[0] for g in graphs]
    assert 0 in sizes and 1 in sizes
    assert any(n > 1 and len(O.undirected_edges(n, e)) == 0 for n, e, _ in graphs)                     # edgeless
    assert any(max(len(x) for x in O.neighbours(n, e)) == 12 for n, e, _ in graphs if n == 13)        # the star: degree M - 1
    assert any(len(np.unique(O.undirected_edges(n, e), axis=0)) < len(O.undirected_edges(n, e)) for n, e, _ in graphs if n)
    assert any(n > 1 and len(set(lab.tolist())) == 1 for n, _, lab in graphs)
    # a 0-node graph has no features: a zero row and column, before and after normalisation
    g0 = sizes.index(0)
    assert not z["small_wl_node"][g0].any() and not z["small_sp_node_norm"][:, g0].any()


def test_c6_and_two_triangles_share_wl_rows_but_not_sp_rows():
    one = np.zeros(6, np.int64)
    graphs = [(6, O.both_ways(O.cycle(6)), one), (6, O.both_ways(O.cycle(3) + O.cycle(3, 3)), one)]
    wl = O.wl_features(graphs, 3).toarray()
    np.testing.assert_array_equal(wl[0], wl[1])
    sp = O.sp_features(graphs).toarray()
    assert not np.array_equal(sp[0], sp[1])
    assert sp[0].sum() == sp[1].sum() == 36            # every ordered pair, k = j and unreachable ones included


def test_label_ranks_of_negative_and_large_labels():
    from kgcn_amd.graph_kernel import dense_label_ranks
    lab = np.array([[2 ** 31 - 1, -5, 0], [-5, -(2 ** 31), 2 ** 31 - 1]], np.int64)
    ranks, count = dense_label_ranks(lab)
    assert ranks.dtype == np.int32 and ranks.shape == lab.shape and count == 4
    np.testing.assert_array_equal(ranks, np.unique(lab, return_inverse=True)[1].reshape(lab.shape))
    np.testing.assert_array_equal(ranks, [[3, 1, 2], [1, 0, 3]])
    empty, none = dense_label_ranks(np.zeros(0, np.int64))
    assert empty.shape == (0,) and none == 0


def test_dataset_graphs_reads_both_adjacency_forms():
    from kgcn_amd.graph_kernel import dataset_graphs
    dense = [np.array([[1, 1, 0], [1, 1, 2], [0, 2, 1]]), np.array([[0, 1], [1, 0]])]
    coo = []
    for a in dense:
        r, c = np.nonzero(a)
        coo.append((np.stack([r, c], 1), a[r, c].astype(np.float32), a.shape))
    node = [np.array([4, -1, 4]), np.array([7, 7, 9])]                # the second graph's row is padded past its 2 nodes
    label = np.array([[1], [0]])
    got = [dataset_graphs({"dense_adj": dense, "node": node, "label": label}),
           dataset_graphs({"adj": coo, "node": node, "label": label})]
    for adjs, nn, labels, y in got:
        np.testing.assert_array_equal(nn, [3, 2])
        np.testing.assert_array_equal(y, label)
        np.testing.assert_array_equal(labels[0], [4, -1, 4])
        np.testing.assert_array_equal(labels[1], [7, 7])
        assert all(tuple(a[0][2]) == (3, 3) for a in adjs)
        lower = [sorted(map(tuple, a[0][0][a[0][0][:, 0] > a[0][0][:, 1]].tolist())) for a in adjs]
        assert lower == [[(1, 0), (2, 1)], [(1, 0)]]
    with pytest.raises(KeyError):
        dataset_graphs({"label": label})


def test_svm_cv_never_fits_on_a_test_graph_and_beats_the_majority_class(z, monkeypatch):
    pytest.importorskip("sklearn")
    import sklearn.svm
    from kgcn_amd.graph_kernel import svm_cv
    graphs, y = O.unpack_graphs(z, "two_"), z["two_y"]
    K = O.normalize(O.wl_gram(graphs, 3))
    perm = np.random.default_rng(0).permutation(len(y))
    K, y = K[np.ix_(perm, perm)], y[perm]
    # rows of K are made recognisable: fit sees K[tr][:, tr], whose row sums identify tr only through the indices we log
    fitted = []
    real_fit = sklearn.svm.SVC.fit

    def spy(self, X, yy, *a, **k):
        fitted.append(X.shape[0])
        return real_fit(self, X, yy, *a, **k)

    monkeypatch.setattr(sklearn.svm.SVC, "fit", spy)
    res = svm_cv(K, y, test_splits=5)
    assert len(res["test_acc"]) == len(res["best_C"]) == len(res["val_acc"]) == 5
    assert len(fitted) == 5 * 5 * 5 and len(res["fit_indices"]) == 25
    folds = [np.arange(len(y))[k * 24:(k + 1) * 24] for k in range(5)]                 # KFold without shuffling, 120 / 5
    for k, tr in enumerate(res["fit_indices"]):
        assert not set(tr.tolist()) & set(folds[k // 5].tolist())
        assert len(tr) == 96 - (20 if (k % 5) == 0 else 19) and len(set(tr.tolist())) == len(tr)
    assert all(n in (76, 77) for n in fitted)
    majority = max(np.mean(y == 0), np.mean(y == 1))
    assert res["mean"] > majority and res["mean"] == pytest.approx(np.mean(res["test_acc"]))
    # one explicit train / test split
    one = svm_cv(K, y, idx_train_val=np.arange(90), idx_test=np.arange(90, 120))
    assert len(one["test_acc"]) == 1 and all(tr.max() < 90 for tr in one["fit_indices"])
