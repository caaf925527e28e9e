"""The host code shared by the graph-kernel, hash-kernel, SVM and label-propagation ops of kgcn_amd/ops.py (the section from
"classical graph kernels" to the end of the file), where the suites of those families do not go:

1. The refusal table.  Every device-tensor operand of every public op of the section, handed over with a wrong dtype, as a
   non-contiguous view and with a wrong element count or shape: the op raises its documented exception class with a message that
   starts "<op>: <operand> must be a contiguous", before anything is launched -- ops.check is not reached, kgcn_last_error does
   not change and no operand (outputs such as lp_select's labels / active / log included) changes a byte.  One row per (op,
   operand) in REFUSALS: a later op adds rows, not a test.  The unbroken call of every op runs once, so that the fault is the
   only thing a refusal can be about.
2. Plain equals copies = 1.  wl_refine / wl_rank / wl_runs / sp_features and their _copies forms are one host body each, the
   plain op being copies = 1 through its own C entry point: the two return the same bytes (run lists and info included) on the
   two-graph case of the table and on one graph of 13 nodes.

Shapes: two graphs of three nodes with one edge each, copies = 2, d = 2, a 3 x 3 Gram, one training set of two rows, one task of
two classes over three points."""
import functools

import numpy as np
import pytest

import graph_kernel_oracle as O

pytestmark = pytest.mark.gpu

GRAPHS = {"two_graphs": [(3, O.both_ways([(1, 0)]), np.array([0, 1, 0])), (3, O.both_ways([(2, 1)]), np.array([1, 0, 0]))],
          "thirteen_nodes": [(13, O.both_ways(O.cycle(13) + [(7, 2), (11, 4), (12, 6)]), np.arange(13) % 3)]}
COPIES = 2


def up(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


@functools.lru_cache(maxsize=None)
def graph_set(name):
    from kgcn_amd import graph_kernel as gk
    adjs, nn, lab = O.to_adjs(GRAPHS[name])
    return gk.GraphSet(adjs, nn, lab)


# ---- the unbroken calls: op -> (the function, its arguments by name, in order) ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def good_calls():
    import torch
    from kgcn_amd import ops
    gs = graph_set("two_graphs")
    nn, (col, count) = gs.num_nodes, gs.initial_colours("node")
    colR = torch.cat([col, col + count])                             # copies with disjoint colours, as hash_graph_kernel makes them
    labR = col.repeat(COPIES)
    nbr, hi, lo = ops.wl_refine(gs.csr, nn, col)
    nbrR, hiR, loR = ops.wl_refine_copies(gs.csr, nn, colR, COPIES)
    runs = ops.wl_runs(col, nn, gs.T, gs.M, 0)
    K = up([[2.0, 0.0, 1.0], [0.0, 2.0, 1.0], [1.0, 1.0, 2.0]])
    train, ev = ops.SvmSets([[0, 1]], [[1, -1]], graphs=3), ops.SvmSets([[2, 0]], graphs=3)
    alpha, rho = ops.svm_smo_batch(K, train, [0], [1.0])[:2]
    dec, job_out, _ = ops.svm_decision_batch(K, train, [0], alpha, rho, ev, [0], [0])
    X = up([[0.0, 0.5], [1.0, -0.5], [0.25, 0.25]])
    W = ops.rbf_affinity(X, 1.0)
    lp_labels = up([[0], [1], [-1]], np.int32)
    dist = ops.lp_propagate(W, ops.lp_degrees(W)[0], lp_labels, [0, 2], ops.LP_PROPAGATION)[0]
    cand = up([1, 2], np.int32)
    x = up(np.arange(12.0).reshape(6, 2) % 5)
    return {
        "wl_refine": (ops.wl_refine, dict(csr=gs.csr, num_nodes=nn, colors=col)),
        "wl_rank": (ops.wl_rank, dict(csr=gs.csr, num_nodes=nn, colors=col, sorted_nbr=nbr, key_hi=hi, key_lo=lo)),
        "wl_runs": (ops.wl_runs, dict(colors=col, num_nodes=nn, T=gs.T, M=gs.M, column_offset=0)),
        "sp_features": (ops.sp_features, dict(csr=gs.csr, num_nodes=nn, labels=col, num_labels=count)),
        "wl_refine_copies": (ops.wl_refine_copies, dict(csr=gs.csr, num_nodes=nn, colors=colR, copies=COPIES)),
        "wl_rank_copies": (ops.wl_rank_copies, dict(csr=gs.csr, num_nodes=nn, colors=colR, copies=COPIES, sorted_nbr=nbrR, key_hi=hiR,
                                                    key_lo=loR)),
        "wl_runs_copies": (ops.wl_runs_copies, dict(colors=colR, num_nodes=nn, T=gs.T, M=gs.M, copies=COPIES, column_offset=0,
                                                    column_stride=1 << 32)),
        "sp_features_copies": (ops.sp_features_copies, dict(csr=gs.csr, num_nodes=nn, labels=labR, copies=COPIES, num_labels=count)),
        "gram_from_runs": (ops.gram_from_runs, dict(run_col=runs[0], run_graph=runs[1], run_count=runs[2], G=gs.T)),
        "gram_normalize": (ops.gram_normalize, dict(K=K)),
        "attr_scale": (ops.attr_scale, dict(x=x)),
        "lsh_buckets": (ops.lsh_buckets, dict(x=x, v=up([[1.0, 0.5], [-0.5, 2.0]]), b=up([0.25, 0.75]), bin_width=1.0)),
        "rank_pairs": (ops.rank_pairs, dict(hi=up([3, -1, 3, 0]), lo=up([0, 5, 0, 0]), mark=up([0, 0, 0, -1], np.int32))),
        "svm_smo_batch": (ops.svm_smo_batch, dict(K=K, sets=train, prob_set=[0], prob_C=[1.0])),
        "svm_decision_batch": (ops.svm_decision_batch, dict(K=K, sets=train, prob_set=[0], alpha=alpha, rho=rho, eval_sets=ev,
                                                            job_prob=[0], job_eval=[0])),
        "svm_vote": (ops.svm_vote, dict(dec=dec, job_out=job_out, eval_sets=ev, vote_first_job=[0], vote_eval=[0], classes=2,
                                        labels=up([0, 1, 1], np.int32))),
        "rbf_affinity": (ops.rbf_affinity, dict(X=X, gamma=1.0)),
        "lp_degrees": (ops.lp_degrees, dict(W=W)),
        "lp_propagate": (ops.lp_propagate, dict(W=W, scale=ops.lp_degrees(W)[0], labels=lp_labels, task_col=[0, 2],
                                                variant=ops.LP_PROPAGATION)),
        "lp_scores": (ops.lp_scores, dict(dist=dist, task_col=[0, 2], cand=cand)),
        "lp_select": (ops.lp_select, dict(score=up([0.5, 0.25]), cand=cand, n=3, k=1, largest=True, active=up([0, 1, 1], np.int32),
                                          labels=lp_labels.clone(), truth=up([[0], [1], [1]], np.int32), log=up([-1], np.int32))),
    }


# ---- the table: (op, operand, the faults it is fed) ------------------------------------------------------------------------------
# "dtype": another dtype; "strided": a non-contiguous view of the same shape and values (not for an operand of one element, which
# is contiguous whatever its strides); "longer": one more entry along the first dimension; "rank": one more dimension in front, for
# an operand whose sizes the op reads from the operand itself, where no size is wrong alone; "wider": one more column, for a
# [rows, d] operand whose rows are open and whose d is not.  run_col of gram_from_runs is read in any shape: its size is what the
# other two are held to.
ALL, OPEN = ("dtype", "strided", "longer"), ("dtype", "strided", "rank")
COLOURS = [("num_nodes", ALL), ("colors", ALL)]
RANK = COLOURS + [("sorted_nbr", ALL), ("key_hi", ALL), ("key_lo", ALL)]
REFUSALS = {
    "wl_refine": COLOURS, "wl_refine_copies": COLOURS, "wl_rank": RANK, "wl_rank_copies": RANK, "wl_runs": COLOURS, "wl_runs_copies": COLOURS,
    "sp_features": [("num_nodes", ALL), ("labels", ALL)], "sp_features_copies": [("num_nodes", ALL), ("labels", ALL)],
    "gram_from_runs": [("run_col", ("dtype", "strided")), ("run_graph", ALL), ("run_count", ALL)],
    "gram_normalize": [("K", ALL)],
    "attr_scale": [("x", OPEN)],
    "lsh_buckets": [("x", OPEN), ("v", OPEN + ("wider",)), ("b", ALL)],
    "rank_pairs": [("hi", OPEN), ("lo", ALL), ("mark", ALL)],
    "svm_smo_batch": [("K", ALL)],
    "svm_decision_batch": [("K", ALL), ("alpha", ALL), ("rho", ("dtype", "longer"))],
    "svm_vote": [("dec", ALL), ("labels", OPEN)],
    "rbf_affinity": [("X", OPEN)],
    "lp_degrees": [("W", ALL)],
    "lp_propagate": [("W", ALL), ("scale", ALL), ("labels", ALL)],
    "lp_scores": [("dist", OPEN + ("wider",)), ("cand", OPEN)],
    "lp_select": [("score", ALL), ("cand", OPEN), ("active", ALL), ("labels", ALL), ("truth", ALL), ("log", ("dtype", "longer"))],
}
ROWS = [(op, operand, fault) for op, operands in REFUSALS.items() for operand, faults in operands for fault in faults]
PUBLIC_OPS = ("wl_refine wl_rank wl_runs sp_features wl_refine_copies wl_rank_copies wl_runs_copies sp_features_copies gram_from_runs "
              "gram_normalize attr_scale lsh_buckets rank_pairs svm_smo_batch svm_decision_batch svm_vote rbf_affinity lp_degrees "
              "lp_propagate lp_scores lp_select").split()


def broken(t, fault):
    import torch
    if fault == "dtype":
        return t.to({torch.float64: torch.float32, torch.int32: torch.int64, torch.int64: torch.int32}[t.dtype])
    if fault == "strided":
        assert t.numel() > 1
        view = torch.stack([t, t], dim=-1)[..., 0]
        assert not view.is_contiguous() and view.shape == t.shape and torch.equal(view, t)
        return view
    if fault == "longer":
        return torch.cat([t, t[:1]]).contiguous()
    if fault == "wider":
        return torch.cat([t, t[:, :1]], dim=1).contiguous()
    assert fault == "rank"
    return t[None].contiguous()


def test_the_table_covers_every_device_operand_of_every_op():
    import torch
    calls = good_calls()
    assert sorted(REFUSALS) == sorted(calls) == sorted(PUBLIC_OPS)
    for op, (_, args) in calls.items():
        assert sorted(name for name, value in args.items() if torch.is_tensor(value)) == sorted(name for name, _ in REFUSALS[op]), op


@pytest.mark.parametrize("op", PUBLIC_OPS)
def test_the_unbroken_call_runs(op):
    import torch
    fn, args = good_calls()[op]
    args = {k: v.clone() if torch.is_tensor(v) else v for k, v in args.items()}       # lp_select teaches its labels
    fn(*args.values())
    torch.cuda.synchronize()


@pytest.mark.parametrize("op,operand,fault", ROWS, ids=["%s-%s-%s" % r for r in ROWS])
def test_refused_before_any_launch(op, operand, fault, monkeypatch):
    import torch
    from kgcn_amd import _lib, ops
    fn, args = good_calls()[op]
    args = {k: v.clone() if torch.is_tensor(v) else v for k, v in args.items()}
    args[operand] = broken(args[operand], fault)
    before = {k: v.clone() for k, v in args.items() if torch.is_tensor(v)}
    last_error = _lib.lib.kgcn_last_error()
    reached = []
    monkeypatch.setattr(ops, "check", lambda rc, what="": reached.append(what))
    with pytest.raises(_lib.KgcnHipError) as info:
        fn(*args.values())
    assert type(info.value) is _lib.KgcnHipError
    assert str(info.value).startswith("%s: %s must be a contiguous " % (op, operand)), str(info.value)
    assert reached == [], "a C entry point was called before the refusal: %s" % reached
    assert _lib.lib.kgcn_last_error() == last_error
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(args[k], v), k


# ---- plain equals copies = 1 -----------------------------------------------------------------------------------------------------
def same_bytes(plain, copies):
    assert len(plain) == len(copies)
    for a, b in zip(plain, copies):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert a.dtype == b.dtype and a.size == b.size
        np.testing.assert_array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


@pytest.mark.parametrize("op", ["wl_refine", "wl_rank", "wl_runs", "sp_features"])
@pytest.mark.parametrize("graphs", sorted(GRAPHS))
def test_plain_is_copies_1(graphs, op):
    from kgcn_amd import ops
    gs = graph_set(graphs)
    nn, (col, count) = gs.num_nodes, gs.initial_colours("node")
    assert gs.M == max(g[0] for g in GRAPHS[graphs]) and count > 1
    nbr, hi, lo = ops.wl_refine(gs.csr, nn, col)
    if op == "wl_refine":
        got = ops.wl_refine_copies(gs.csr, nn, col, 1)
        assert nbr.shape == (gs.csr.nnz,) and got[0].shape == (1, gs.csr.nnz) and hi.shape == got[1].shape == (gs.T * gs.M,)
        same_bytes((nbr, hi, lo), got)
    elif op == "wl_rank":
        new, info = ops.wl_rank(gs.csr, nn, col, nbr, hi, lo)
        assert info.tolist()[0] > count and info.tolist()[1] == 0        # the refinement split a colour
        same_bytes((new, info), ops.wl_rank_copies(gs.csr, nn, col, 1, nbr[None], hi, lo))
    elif op == "wl_runs":
        new = ops.wl_rank(gs.csr, nn, col, nbr, hi, lo)[0]
        plain = ops.wl_runs(new, nn, gs.T, gs.M, 5 << 32)
        assert int(plain[2].sum().item()) == int(gs.num_nodes_host.sum())
        same_bytes(plain, ops.wl_runs_copies(new, nn, gs.T, gs.M, 1, 5 << 32, 9 << 32))
    else:
        plain = ops.sp_features(gs.csr, nn, col, count)
        assert int(plain[2].sum().item()) == int((gs.num_nodes_host ** 2).sum())
        same_bytes(plain, ops.sp_features_copies(gs.csr, nn, col, 1, count))
