"""CPU checks of knowledge-graph link prediction: the fp64 oracle (tests/linkpred_oracle.py) against a plain loop transcription
and finite differences, the fixture g8_kg_linkpred.npz against a regeneration, the loader, and the host negative draw."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import linkpred_oracle as O  # noqa: E402
import vae_oracle as V  # noqa: E402

MODES = ("gcn", "distmult", "ip")
GOLDEN = os.path.join(ROOT, "tests", "golden", "g8_kg_linkpred.npz")


def _case(rng, N=12, D=5, L=9, R=3, scale=1.0):
    h = rng.standard_normal((N, D)) * scale
    w = rng.standard_normal((R, D))
    rows = np.stack([rng.integers(0, N, L), rng.integers(0, R, L), rng.integers(0, N, L),
                     rng.integers(0, N, L), rng.integers(0, R, L), rng.integers(0, N, L)], axis=1)
    rows[:, 3] = rows[:, 0]
    return h, w, rows


def _loop_loss(h, w, rows, mode):
    """Line by line, one row at a time, as the model files write it."""
    s1, s2 = [], []
    for i0, r1, j0, i1, r2, j1 in rows:
        a = sum(h[i0, d] * h[j0, d] * (w[r1, d] if mode == "distmult" else 1.0) for d in range(h.shape[1]))
        b = sum(h[i1, d] * h[j1, d] * (w[r2, d] if mode == "distmult" else 1.0) for d in range(h.shape[1]))
        s1.append(a)
        s2.append(b)
    if mode == "ip":
        S1, S2 = sum(s1), sum(s2)
        c = -np.log(1.0 / (1.0 + np.exp(S2 - S1 + 0.1)) + 1e-10)
        return c, c, float(S1 > S2)
    cost = []
    for a, b in zip(s1, s2):
        y = 1.0 / (1.0 + np.exp(-(a - b))) if mode == "gcn" else 1.0 / (1.0 + np.exp(b - a + 0.1))
        cost.append(-np.log(y + 1e-10))
    return sum(cost) / len(cost), sum(cost), float(sum(a > b for a, b in zip(s1, s2)))


@pytest.mark.parametrize("mode", MODES)
def test_oracle_loss_matches_loop_transcription(mode):
    rng = np.random.default_rng(1)
    h, w, rows = _case(rng)
    res = O.loss(*O.scores(h, rows, mode, w), mode)
    ref = _loop_loss(h, w, rows, mode)
    assert np.allclose([res["cost_opt"], res["cost_sum"], res["correct_count"]], ref, rtol=1e-12, atol=0)


def _objective(h, w, rows, mode, g_opt, g_sum):
    r = O.loss(*O.scores(h, rows, mode, w), mode)
    return g_opt * r["cost_opt"] + g_sum * r["cost_sum"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scale", [0.5, 6.0])
def test_oracle_gradients_against_finite_differences(mode, scale):
    """scale 6: |s2 - s1| of tens, where 1 - sigmoid and the +1e-10 term shape the derivative."""
    rng = np.random.default_rng(2)
    h, w, rows = _case(rng, scale=scale)
    g_opt, g_sum = 0.7, 0.3
    dh, dw = O.loss_grads(h, rows, mode, w, g_opt, g_sum)
    eps = 1e-6
    for arr, grad in ((h, dh),) + (((w, dw),) if mode == "distmult" else ()):
        num = np.zeros_like(arr)
        for idx in np.ndindex(arr.shape):
            old = arr[idx]
            arr[idx] = old + eps
            fp = _objective(h, w, rows, mode, g_opt, g_sum)
            arr[idx] = old - eps
            fm = _objective(h, w, rows, mode, g_opt, g_sum)
            arr[idx] = old
            num[idx] = (fp - fm) / (2 * eps)
        assert np.abs(num - grad).max() <= 1e-6 * max(1.0, np.abs(num).max()), np.abs(num - grad).max()


def test_plus_1e10_region_and_overflow_limit():
    # s2 - s1 = 30: sigmoid(-30) ~ 9e-14 << 1e-10, so the derivative is y (1 - y) / (y + 1e-10) ~ 1e-3 y, not 1 - y
    s1, s2 = np.array([0.0]), np.array([30.0])
    for mode in ("gcn", "distmult"):
        f = lambda x: float(O.pair_cost(x, s2, mode)[0])
        num = (f(s1 + 1e-3) - f(s1 - 1e-3)) / 2e-3
        ana = float(O.pair_dcost(s1, s2, mode)[0])
        assert abs(num - ana) <= 1e-6 * max(1e-12, abs(num)) + 1e-15, (mode, num, ana)
        assert abs(ana) < 1e-3
    # beyond fp32's exp range: the cost is -log(1e-10), the derivative the defined limit 0 (fp64 would still be finite)
    s1, s2 = np.array([0.0]), np.array([100.0])
    assert np.isclose(O.pair_cost(s1, s2, "distmult")[0], -np.log(1e-10))
    assert O.pair_dcost(s1, s2, "distmult")[0] == 0.0
    assert O.pair_dcost(s1, s2, "distmult", f32_limit=False)[0] != 0.0


def test_negative_draw_hand_cases():
    # round 0 of row i, step s is Philox block (i, s, 0, 0): the words of vae_oracle's (numpy-checked) generator
    words = V.philox_blocks(7, 3, 4)
    for K in (1, 2, 5000, 2 ** 31 - 1):
        t = (2 ** 64 - K) % K
        got = O.draw_indices(7, 3, range(4), K)
        for i in range(4):
            ok = [int(x) for x in words[i] if (int(x) * K) % 2 ** 64 >= t]
            assert got[i] == (ok[0] * K) >> 64
    assert np.array_equal(O.draw_indices(7, 3, range(4), 1), np.zeros(4))
    # K = 2^63 + 1: 2^64 mod K = 2^63 - 1, about half of the words are rejected -- the later ones (and rounds) are used
    K = 2 ** 63 + 1
    got = O.draw_indices(5, 0, range(64), K)
    assert all(0 <= int(g) < K for g in got.astype(object))
    # uniform on a small table
    u = O.draw_indices(11, 1, range(6000), 3)
    assert abs(np.bincount(u, minlength=3) / 6000.0 - 1 / 3).max() < 0.03


def test_assemble_restates_the_feed():
    rng = np.random.default_rng(4)
    lab = rng.integers(0, 50, (40, 6))
    perm = rng.permutation(40)
    neg = np.unique(np.concatenate([lab[:, 0], lab[:, 2]]))
    rows = O.assemble(lab, perm, neg, 8, 9, 6)                 # window 6 mod 5 = 1
    src = lab[perm[8:16]]
    assert np.array_equal(rows[:, [0, 1, 2, 4]], src[:, [0, 1, 2, 4]])
    assert np.array_equal(rows[:, 3], src[:, 0])
    assert np.array_equal(rows[:, 5], neg[O.draw_indices(9, 6, range(8), len(neg))])


# ---- fixture and loader ------------------------------------------------------------------------------------------------------
def test_fixture_shape():
    z = np.load(GOLDEN)
    assert int(z["node_num"]) == 5000 and z["label_list"].shape == (1, 39920, 6) and z["test_label_list"].shape == (1, 9980, 6)
    assert z["adj_idx"].shape == (44920, 2) and list(z["relation_ids"]) == [0, 1, 2]


def test_oracle_preprocessing_reproduces_the_fixture_draws():
    """The oracle's restatement of preprocessing_link_pred.py, run on the fixture's own positive edges, reproduces its lists."""
    z = np.load(GOLDEN)
    N = int(z["node_num"])
    lab, test = z["label_list"][0], z["test_label_list"][0]
    names = {0: "negative", 1: "self", 2: "interaction"}
    # the edge files of the split as load_graph reads them back: node names are the decimal ids of the BA network, and the
    # sorted name order maps them to 0 .. N-1 in string order
    adj = z["adj_idx"]
    train_pairs = adj[adj[:, 0] != adj[:, 1]]
    strs = sorted(str(i) for i in range(N))
    name_of = {i: s for i, s in enumerate(strs)}
    train_lines = ["%s\t%s\t%s" % (name_of[a], names[2], name_of[b]) for a, b in train_pairs]
    test_pos = set(map(tuple, test[:, :3]))
    test_lines = ["%s\t%s\t%s" % (name_of[a], names[r], name_of[b]) for a, r, b in sorted(test_pos)]
    out = O.preprocess(train_lines, test_lines, 0)
    assert out["node_num"] == N
    assert np.array_equal(out["adj_idx"], adj.astype(np.int64))
    assert np.array_equal(out["label_list"], z["label_list"].astype(np.int64))
    assert np.array_equal(out["test_label_list"], z["test_label_list"].astype(np.int64))


def test_loader_on_the_fixture():
    from kgcn_amd import data_util as D
    z = np.load(GOLDEN)
    data = {"adj": [(z["adj_idx"], z["adj_val"], np.array([5000, 5000]))], "node": z["node"], "node_num": z["node_num"],
            "label_list": z["label_list"], "test_label_list": z["test_label_list"]}
    d = D.LinkPredictionData(data)
    assert d.num_nodes == 5000 and d.num_relations == 3
    ch = d.channels[0]
    assert len(d.channels) == 1 and np.array_equal(np.stack([ch.row, ch.col], 1), z["adj_idx"])
    assert np.array_equal(d.label_list, z["label_list"][0])
    neg = D.all_label(d.label_list)
    assert np.array_equal(neg, np.unique(np.concatenate([d.label_list[:, 0], d.label_list[:, 2]])))
    bad = dict(data, node=z["node"][:, ::-1])
    with pytest.raises(ValueError):
        D.LinkPredictionData(bad)
    bad = dict(data, label_list=z["label_list"].copy())
    bad["label_list"][0, 3, 2] = 5000
    with pytest.raises(ValueError):
        D.LinkPredictionData(bad)


def test_split_label_list_restates_the_reference():
    from kgcn_amd import data_util as D
    lab = np.arange(60).reshape(10, 6)
    tr, va = D.split_label_list(lab, 0.2, np.random.RandomState(3))
    nid = np.arange(10)
    np.random.RandomState(3).shuffle(nid)
    assert np.array_equal(tr, lab[nid[:8]]) and np.array_equal(va, lab[nid[8:]])
