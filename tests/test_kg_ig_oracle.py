"""The algebra behind csrc/kgig.hip, proven in fp64 before any kernel runs (tests/kg_ig_oracle.py): the restructured formulas give
what the reference's loop gives, integrated gradients are complete in the limit, and the host-side pieces (validation, the dump's
BFS and normalisation, the closed form of the table models) do what they say.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kg_ig_oracle as O  # noqa: E402
import linkpred_oracle as LO  # noqa: E402

N = 70


@pytest.fixture(scope="module")
def graph():
    idx, val = O.make_graph(N)
    return LO.dense_adj(idx, val, N)


@pytest.fixture(scope="module")
def params():
    return O.random_params(N)


def _rel(x, y):
    return float(np.abs(x - y).max() / np.abs(y).max())


@pytest.mark.parametrize("mode,target", [
    (O.SCORE, (5, 9, -1, -1)), (O.SCORE, (7, 7, -1, -1)), (O.SCORE, (0, 1, -1, -1)),          # a == b; the hub and the self-loop row
    (O.LOSS, (5, 9, 5, 30)), (O.LOSS, (3, 3, 3, 40)), (O.LOSS, (59, 0, 64, 0)), (O.LOSS, (20, 21, 21, 40)),    # the hub / node 21 on both sides
    (O.SCORE, "node")])
def test_restructured_equals_literal(graph, params, mode, target):
    if target == "node":                                    # visualize_type 'node': node t and its best partner, score mode
        target = (13, O.node_partner(params, graph, 13), -1, -1)
    scales, weights = O.reference_scales(6)
    lit = O.literal(params, graph, target, mode, scales, weights)
    res = O.restructured(params, graph, target, mode, scales, weights)
    assert np.abs(lit["ig"]).max() > 0
    for key in ("ig", "u", "node_ig", "score"):
        assert _rel(res[key], lit[key]) < 1e-12, key
    assert _rel(res["ig"].sum(-1), res["node_ig"]) < 1e-12            # the node-reduced form needs no [N, C] product


@pytest.mark.parametrize("mode,target", [(O.SCORE, (5, 9, -1, -1)), (O.LOSS, (5, 9, 5, 30))])
def test_completeness_improves_with_steps(graph, params, mode, target):
    want = O.score_at(params, graph, target, mode, 1.0) - O.score_at(params, graph, target, mode, 0.0)
    gaps = []
    for K in (8, 64, 512):
        scales, weights = O.reference_scales(K)
        gaps.append(abs(O.restructured(params, graph, target, mode, scales, weights)["ig"].sum() - want))
    assert gaps[0] > gaps[1] > gaps[2], gaps
    assert gaps[2] < 0.02 * abs(want), (gaps, want)


def test_asymmetric_values_matter(graph, params):
    """A^T for A, or unit values, gives another answer on this graph: the fixtures can tell such a mistake."""
    scales, weights = O.reference_scales(4)
    ref = O.literal(params, graph, (5, 9, -1, -1), O.SCORE, scales, weights)["node_ig"]
    for other in (graph.T.tocsr(), (graph != 0).astype(np.float64).tocsr()):
        assert _rel(O.literal(params, other, (5, 9, -1, -1), O.SCORE, scales, weights)["node_ig"], ref) > 1e-3


# ---- the table models ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", [(3, 8), (4, 4)])
@pytest.mark.parametrize("with_w", [False, True])
def test_closed_form_of_the_table_models(a, b, with_w):
    rng = np.random.RandomState(3)
    E = rng.uniform(-0.5, 0.5, (12, 8))
    w = rng.standard_normal(8) if with_w else None
    scales, weights = O.reference_scales(30)
    lit = O.literal_table(E, w, a, b, scales, weights)
    assert _rel(O.closed_table(E, w, a, b, scales, weights), lit) < 1e-12


@pytest.mark.parametrize("variant", ["distmult", "ip"])
def test_table_models_through_the_public_function(variant):
    import torch
    from kgcn_amd import models, visualization as V
    torch.manual_seed(0)
    model = models.LinkPredictionNet(variant, 12, num_relations=3, embedding_dim=8)
    labels = np.array([[3, 2, 8, 3, 0, 5], [4, 1, 4, 4, 0, 6]], np.int64)
    out = V.linkpred_integrated_gradients(model, None, labels, "edge_score", divide_number=30, reduce=None)
    E = model.embedding.detach().numpy().astype(np.float64)
    scales, weights = V.ig_scales("ig", 30)
    for rec, row in zip(out, labels):
        w = model.distmult.w[0][row[1]].detach().numpy().astype(np.float64) if variant == "distmult" else None
        lit = O.literal_table(E, w, row[0], row[2], scales, weights)
        assert _rel(rec["ig"], lit) < 1e-5
        assert rec["vis_nodes"] == [row[0], row[2]]
        assert abs(rec["sum_of_ig"] - lit.sum()) < 1e-5 * np.abs(lit).max() * lit.size
    for kind in ("edge_loss", "node"):
        with pytest.raises(ValueError, match="model_py/gcn.py only"):
            V.linkpred_integrated_gradients(model, None, labels, kind)


# ---- the dump ----------------------------------------------------------------------------------------------------------------
def test_dump_on_a_hand_worked_graph(tmp_path):
    """0 -> 0, 0 -> 1, 1 -> 2, 2 -> 3, 3 -> 4, 4 -> 5, 5 -> 5 (directed as stored; the dump's graph is undirected)."""
    from kgcn_amd import visualization as V
    indptr, indices = np.array([0, 2, 3, 4, 5, 6, 7]), np.array([0, 1, 2, 3, 4, 5, 5])
    nodes, edges = V.kg_subgraph(indptr, indices, [2], 1)
    assert nodes.tolist() == [1, 2, 3] and edges.tolist() == [[1, 2], [2, 3]]
    nodes, edges = V.kg_subgraph(indptr, indices, [2], 2)
    assert nodes.tolist() == [0, 1, 2, 3, 4] and edges.tolist() == [[0, 0], [0, 1], [1, 2], [2, 3], [3, 4]]
    nodes, edges = V.kg_subgraph(indptr, indices, [0, 5], 1)
    assert nodes.tolist() == [0, 1, 4, 5] and edges.tolist() == [[0, 0], [0, 1], [4, 5], [5, 5]]
    nodes, edges = V.kg_subgraph(indptr, indices, [3], 0)
    assert nodes.tolist() == [3] and edges.tolist() == []
    ig = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    rec = {"target": 0, "vis_nodes": [2, 3], "node_ig": ig}
    (ef, nf), = V.dump_kg(rec, (indptr, indices), str(tmp_path), 1)
    assert os.path.basename(ef) == "edgepred-2-3-edge.csv" and os.path.basename(nf) == "edgepred-2-3-node.csv"
    assert open(ef).read().split() == ["1,2", "2,3", "3,4"]
    lines = open(nf).read().split()
    assert lines[0] == "label,ig" and [ln.split(",")[0] for ln in lines[1:]] == ["1", "2", "3", "4"]
    std = np.sqrt(35.0 / 12.0)                               # population std of 1..6, mean 3.5
    got = np.array([float(ln.split(",")[1]) for ln in lines[1:]])
    assert np.allclose(got, (np.array([2.0, 3.0, 4.0, 5.0]) - 3.5) / std, rtol=1e-12, atol=0)
    (ef, nf), = V.dump_kg({"target": 4, "vis_nodes": [4], "node_ig": ig}, (indptr, indices), str(tmp_path), 1)
    assert os.path.basename(nf) == "nodepred-4-node.csv"
    assert open(ef).read().split() == ["3,4", "4,5", "5,5"]


# ---- host validation ------------------------------------------------------------------------------------------------------
def test_host_validation():
    from kgcn_amd import ops
    indptr, indices = np.array([0, 2, 3, 4]), np.array([0, 2, 1, 0])
    tg = np.array([[0, 2, -1, -1]])
    assert ops.kg_ig_check_host(indptr, indices, 3, tg, "score", 30).dtype == np.int32
    bad = [
        dict(indices=np.array([2, 0, 1, 0])),                                  # unsorted row
        dict(indices=np.array([2, 2, 1, 0])),                                  # duplicate column
        dict(indices=np.array([0, 3, 1, 0])),                                  # column out of range
        dict(indptr=np.array([0, 3, 2, 4])),                                   # offsets not monotone
        dict(indptr=np.array([0, 2, 3, 5])),                                   # offsets beyond nnz
        dict(targets=np.array([[0, 3, -1, -1]])),                              # node id out of range
        dict(targets=np.array([[0, 2, -1, -1]]), mode="loss"),                 # loss mode reads all four
        dict(targets=np.array([[0, 2, 1]])),
        dict(targets=np.array([[0.0, 2.0, 1.0, 1.0]])),
        dict(steps=0), dict(width=64), dict(mode="node"), dict(num_nodes=ops.KG_IG_MAX_NODES + 1),
    ]
    for kw in bad:
        args = dict(indptr=indptr, indices=indices, num_nodes=3, targets=tg, mode="score", steps=30, width=128)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.kg_ig_check_host(**args)
    # a first column equal to the previous row's last one is no duplicate; empty rows are legal
    ops.kg_ig_check_host(np.array([0, 1, 1, 2]), np.array([1, 1]), 3)


def test_entry_point_refuses_bad_shapes_before_any_launch():
    from kgcn_amd import _lib
    lib = _lib.lib

    def call(nodes=70, width=128, steps=30, targets=1, mode=0, groups=0):
        return lib.kgcn_kg_ig_f32(None, None, None, 0, nodes, width, None, None, None, None, None, None, None, None, steps, None,
                                  targets, mode, groups, None, None, None, None)
    assert call(targets=0) == 0                                                 # nothing to do
    for kw in (dict(width=64), dict(nodes=0), dict(nodes=7169), dict(steps=0), dict(steps=4097), dict(mode=2),
               dict(targets=-1), dict(groups=-1), dict()):                      # the last: NULL operands
        assert call(**kw) != 0, kw
        assert lib.kgcn_last_error()
    assert call(nodes=5000) != 0 and b"NULL" in lib.kgcn_last_error()           # N = 5,000 passes the size checks


def test_public_function_argument_errors():
    from kgcn_amd import models, visualization as V
    model = models.LinkPredictionNet("ip", 12, embedding_dim=8)
    labels = np.array([[3, 0, 8, 3, 0, 5]], np.int64)
    with pytest.raises(ValueError):
        V.linkpred_integrated_gradients(model, None, labels, "edge")
    with pytest.raises(ValueError):
        V.linkpred_integrated_gradients(model, None, labels, "edge_score", target=1)
    with pytest.raises(ValueError):
        V.linkpred_integrated_gradients(model, None, labels, "edge_score", reduce="sum")
    with pytest.raises(TypeError):
        V.linkpred_integrated_gradients(object(), None, labels)
