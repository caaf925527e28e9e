"""numpy restatement of the link-prediction ranking of the reference (sample_kg/network_prediction/script/predscore.py, what
run_enrichment.sh runs with --train --mode infer): the label pair sets (:40-92), the score-ordered pair list (:126-168), its
train / test / new marks (:194-214), the score ranking (:231-251) and the enrichment counts (:254-280).  Scores are taken in
fp64 unless the caller hands in a matrix of its own.  Test infrastructure only."""
import numpy as np


# ---- label pairs (:40-92) ------------------------------------------------------------------------------------------------
def label_pairs(label_list):
    """:52-60 / :81-89: columns 0 and 2 of every row of label_list[0], each pair sorted, duplicates removed.  The reference
    leaves a Python set's order; here the pairs are sorted -> list of (small, large) tuples."""
    rows = np.asarray(label_list)
    rows = rows[0] if rows.ndim == 3 else rows
    return sorted(set(tuple(sorted((int(r[0]), int(r[2])))) for r in rows))


def target_pairs(label_list, test_label_list):
    """:76-90 (infer): the train and test lists appended along axis 1, then as label_pairs."""
    both = np.append(np.asarray(label_list), np.asarray(test_label_list), axis=1)       # :79
    return label_pairs(both)


# ---- the ordered list (:126-168) -----------------------------------------------------------------------------------------
def pair_scores(h, w=None):
    """The model's lp_prediction in fp64: H H^T, or H diag(w) H^T for one DistMult relation."""
    h = np.asarray(h, np.float64)
    return (h if w is None else h * np.asarray(w, np.float64)) @ h.T


def pair_bounds(h, w=None):
    """sum_k |h_ik w_k h_jk| in fp64: the magnitude an fp32 evaluation's rounding error is relative to."""
    h = np.abs(np.asarray(h, np.float64))
    return (h if w is None else h * np.abs(np.asarray(w, np.float64))) @ h.T


def sort_prediction_score(matrix, cutoff):
    """:142-168: every (matrix[row, col], row, col) with row < col, sorted in reverse as tuples -- score, then row, then col,
    all descending -- and cut to the first `cutoff` (0: all).  Python compares -0.0 == 0.0, so the two tie; a NaN makes
    Python's order undefined: here it ranks below every number (NaNs among themselves by row, col), and a zero is returned
    as +0.0, a NaN as the canonical quiet NaN.  -> (score, row, col) in the matrix's dtype / int32."""
    matrix = np.asarray(matrix)
    n = matrix.shape[0]
    row, col = np.triu_indices(n, 1)                                                       # :144
    s = matrix[row, col]
    order = np.lexsort((-col, -row, -s))                                                   # :153, NaN sorts last
    if cutoff:
        order = order[:cutoff]                                                             # :164
    s = s[order] + s.dtype.type(0)
    s = np.where(np.isnan(s), s.dtype.type(np.nan), s)
    return s, row[order].astype(np.int32), col[order].astype(np.int32)


# ---- convert (:194-214), process_table (:231-251), enrichment (:254-280) -----------------------------------------------------
def convert(row, col, target, test):
    """:201-214 (train): (train_edge, test_edge, new_edge) per entry."""
    target, test = set(target), set(test)
    tr = np.zeros(len(row), np.int64)
    te = np.zeros(len(row), np.int64)
    nw = np.zeros(len(row), np.int64)
    for p, pair in enumerate(zip(row.tolist(), col.tolist())):
        if pair in target:
            if pair in test:
                te[p] = 1
            else:
                tr[p] = 1
        else:
            nw[p] = 1
    return tr, te, nw


def score_ranking(score):
    """:245: len - rankdata(score, 'max') + 1.  rankdata's 'max' rank of x is the number of entries <= x, so this is 1 + the
    number of entries with a strictly larger score."""
    s = np.sort(np.asarray(score))
    return len(s) - np.searchsorted(s, score, side="right") + 1


def enrichment(num_nodes, target, test, train_edge, test_edge, top=tuple(float(p) for p in range(1, 11))):
    """:256-280 -> dict of the printed numbers; per percentage also `covered`: whether the table without train edges has
    top_ratio rows (the reference's iloc silently takes fewer)."""
    train = set(target) - set(test)                                                        # :256
    total = int((1 + (num_nodes - 1)) * (num_nodes - 1) / 2)                               # :258
    out = dict(total=total, total_wo_train=total - len(train), total_target_edges=len(target), total_train_edges=len(train),
               total_test_edges=len(test), top=[], top_ratio=[], test_edges_in_toplist=[], enrichment=[], covered=[])
    kept = np.asarray(test_edge)[np.asarray(train_edge) == 0]                              # :261
    for i in top:
        ratio = i * 0.01                                                                   # :272
        top_ratio = round(out["total_wo_train"] * ratio)                                   # :273
        hits = int(kept[:top_ratio].sum())                                                 # :274-275
        out["top"].append(i)
        out["top_ratio"].append(top_ratio)
        out["test_edges_in_toplist"].append(hits)
        out["enrichment"].append(hits / len(test))                                         # :276
        out["covered"].append(len(kept) >= top_ratio)
    return out


def rank_links(h, label_list, test_label_list, w=None, cutoff=10000, matrix=None):
    """main() :310-338 without the node names -> dict of the table columns and the enrichment numbers."""
    test = label_pairs(test_label_list)
    target = target_pairs(label_list, test_label_list)
    matrix = pair_scores(h, w) if matrix is None else matrix
    score, row, col = sort_prediction_score(matrix, cutoff)
    tr, te, nw = convert(row, col, target, test)
    out = dict(score=score, row=row, col=col, train_edge=tr, test_edge=te, new_edge=nw, score_ranking=score_ranking(score))
    out.update(enrichment(np.asarray(h).shape[0], target, test, tr, te))
    return out
