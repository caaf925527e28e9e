"""The ranking stage of the link-prediction sample (sample_kg/network_prediction/run_enrichment.sh -> script/predscore.py
--train --mode infer): all node pairs in score order, each marked train / test / new edge, and the share of the held-out test
edges found in the top 1 % .. 10 % of the ranking without train edges (the "enrichment").

The reference sorts a Python list of all N (N - 1) / 2 (score, row, col) tuples cut from the dense [N, N] prediction and probes
Python sets per entry.  Here the list is taken from the node rows H [N, D] on the device (ops.pair_rank, csrc/pairrank.hip: the
score matrix is never formed) and marked, ranked and counted there (ops.pair_rank_table); only the label pair sets (a few
thousand pairs) and the ten thresholds are host work.

Deviations from the reference:
  * only its live branch (--train: train edges stay in the list) exists; the other one ends in sys.exit(1) there;
  * ties are in the order of the reference's first sort (score, then row, then col, descending); its later
    DataFrame.sort_values is an unstable sort and leaves the order of tied scores undefined;
  * the two label-set files are written in sorted order; the reference iterates a Python set;
  * for distmult ONE relation is ranked (H diag(w_r) H^T); the reference indexes the [R, N, N] prediction as if it were [N, N];
  * the score is the ranking kernel's own fp32 Gram entry (k ascending, the row operand scaled by w first), not the bits of
    LinkPredictionNet.predict's GEMM;
  * -0.0 ranks as +0.0 (Python compares them equal) and is written as 0.0; a NaN score ranks below every number (Python's
    tuple sort with a NaN in the list has no defined order);
  * N <= 65,536 (a pair is packed as row << 16 | col) and D <= 256.
"""
import numpy as np
import torch

from . import ops

TOP_PERCENT = tuple(float(p) for p in range(1, 11))                   # predscore.py:270


def label_pairs(label_list):
    """predscore.py:40-92: columns 0 and 2 of every row of the label list ([1, M, 6] or [M, 6]), each pair sorted, duplicates
    removed -> int64 [P, 2] in sorted order."""
    rows = np.asarray(label_list)
    rows = rows[0] if rows.ndim == 3 else rows
    if rows.ndim != 2 or rows.shape[1] < 3:
        raise ValueError("label_pairs: the label list must be [1, M, >= 3] or [M, >= 3], got %s" % (np.asarray(label_list).shape,))
    if rows.shape[0] == 0:
        return np.zeros((0, 2), np.int64)
    p = np.sort(rows[:, [0, 2]].astype(np.int64), axis=1)
    return np.unique(p, axis=0)


def top_ratios(total_wo_train, top=TOP_PERCENT):
    """predscore.py:271-273: round(total_wo_train * (p * 0.01)) with Python's own round -- banker's rounding of a float
    product, exactly as the reference computes it."""
    return [round(total_wo_train * (p * 0.01)) for p in top]


class LinkRanking:
    """What predscore.py puts in its table and prints.  Per entry (device tensors, list order): row, col, score,
    score_ranking, train_edge, test_edge, new_edge.  Counts (host): total, total_wo_train, total_target_edges,
    total_train_edges, total_test_edges.  Per percentage of `top` (host lists): top_ratio, test_edges_in_toplist, enrichment,
    covered (False where the list holds fewer than top_ratio entries that are no train edge: the count is then that of a
    shorter table, as in the reference, which does not say so).  test_pairs / train_pairs: int64 [P, 2], sorted."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def lines(self):
        """The enrichment lines, as predscore.py:262-280 prints them."""
        out = ["#total as scored: %d" % self.total, "#total_w/o_train_edges: %d" % self.total_wo_train,
               "#total_target_edges: %d" % self.total_target_edges, "#total_train_edges: %d" % self.total_train_edges,
               "#total_test_edges: %d" % self.total_test_edges]
        for p, r, n, e, c in zip(self.top, self.top_ratio, self.test_edges_in_toplist, self.enrichment, self.covered):
            out.append("#top%%: %s  #top_ratio: %d  #test_edges_in_toplist: %d  #test edges enrichment top%s%%: %s%s"
                       % (p, r, n, p, e, "" if c else "  (the list is shorter than top_ratio: raise the cutoff)"))
        return out


def rank_links(h, label_list, test_label_list, w=None, cutoff=10000, top=TOP_PERCENT):
    """predscore.py main() :310-338 for the node rows h [N, D] (a float32 device tensor; w: one relation's DistMult vector or
    None) -> LinkRanking.  cutoff: the entries kept (0: all pairs), predscore.py's --cutoff."""
    N = int(h.shape[0])
    test = label_pairs(test_label_list)
    both = [np.asarray(x)[0] if np.asarray(x).ndim == 3 else np.asarray(x) for x in (label_list, test_label_list)]
    target = label_pairs(np.concatenate([b[:, :3] for b in both], axis=0))                  # :79: the two lists appended
    for p in (test, target):
        if p.size and (p.min() < 0 or p.max() >= N or np.any(p[:, 0] == p[:, 1])):
            raise ValueError("rank_links: a label pair names a node outside [0, %d) or a node with itself" % N)
    target_codes, test_codes = ops.pair_codes(target, h.device), ops.pair_codes(test, h.device)
    test_set = set(map(tuple, test.tolist()))
    train = np.asarray([p for p in target.tolist() if tuple(p) not in test_set], np.int64).reshape(-1, 2)    # :256
    total = int((1 + (N - 1)) * (N - 1) / 2)                                                 # :258
    total_wo_train = total - len(train)                                                     # :259
    ratios = top_ratios(total_wo_train, top)
    score, row, col = ops.pair_rank(h, w, cutoff)
    train_edge, test_edge, new_edge, ranking, hits, covered = ops.pair_rank_table(score, row, col, target_codes, test_codes, ratios)
    hits = hits.tolist()
    return LinkRanking(row=row, col=col, score=score, score_ranking=ranking, train_edge=train_edge, test_edge=test_edge,
                       new_edge=new_edge, total=total, total_wo_train=total_wo_train, total_target_edges=len(target),
                       total_train_edges=len(train), total_test_edges=len(test), top=list(top), top_ratio=ratios,
                       test_edges_in_toplist=hits, enrichment=[n / len(test) if len(test) else float("nan") for n in hits],
                       covered=[bool(c) for c in covered.tolist()], test_pairs=test, train_pairs=train)


def _names(node_names, n):
    if node_names is None:
        return [str(i) for i in range(n)]
    if isinstance(node_names, str):                                                          # build_node_list, :26-37
        with open(node_names) as f:
            return [line.strip() for line in f]
    return list(node_names)


def write_score_table(result, path, node_names=None):
    """The reference's score file (predscore.py:248-249, :343): tab-separated, header row / col / gene1 / gene2 / score /
    score_ranking / train_edge / test_edge / new_edge, one line per entry in list order.  node_names: a list, or the path of a
    file with one name per line (dataset_node.csv); None: the node ids.  The score is written as the shortest text that reads
    back as the same float32; score_ranking is a float column there (rankdata), written "%.1f"."""
    row, col = result.row.cpu().numpy(), result.col.cpu().numpy()
    score, rank = result.score.cpu().numpy(), result.score_ranking.cpu().numpy()
    tr, te, nw = (t.cpu().numpy() for t in (result.train_edge, result.test_edge, result.new_edge))
    names = _names(node_names, int(max(row.max(), col.max())) + 1)
    with open(path, "w") as f:
        f.write("row\tcol\tgene1\tgene2\tscore\tscore_ranking\ttrain_edge\ttest_edge\tnew_edge\n")
        for p in range(len(row)):
            f.write("%d\t%d\t%s\t%s\t%s\t%.1f\t%d\t%d\t%d\n" % (row[p], col[p], names[row[p]], names[col[p]], score[p], rank[p],
                                                             tr[p], te[p], nw[p]))


def write_label_sets(result, test_path, train_path, node_names=None):
    """output_test_train (predscore.py:95-123, :348-352): the test and the train pairs as two-column tab-separated files of
    node names without a header, in sorted order."""
    pairs = np.concatenate([result.test_pairs, result.train_pairs])
    names = _names(node_names, int(pairs.max()) + 1 if pairs.size else 0)
    for path, part in ((test_path, result.test_pairs), (train_path, result.train_pairs)):
        with open(path, "w") as f:
            for a, b in part.tolist():
                f.write("%s\t%s\n" % (names[a], names[b]))
