#!/usr/bin/env python3
"""Generate tests/golden/g10_predscore.npz by IMPORTING the reference's ranking script in place
(sample_kg/network_prediction/script/predscore.py; nothing of it is copied, only the arrays and printed counts its functions
produce).  The script's main() is followed with --mode infer --train and one process: build_test_label_pairs,
build_target_label_pairs, sort_prediction_score, convert, process_table, enrichment, on a tiny case written to temporary
.jbl files:

  H [40, 8] with entries k / 64, k an integer in [-64, 64] from default_rng(49), a row redrawn while it would repeat a pair
  score: H H^T is exact in fp32 (asserted), and all 780 pair scores are distinct (asserted), so the unstable sort of
  process_table cannot show;
  150 distinct pairs, 120 in the train label list and 30 in the test label list, a third of the rows stored as (larger,
  smaller) and some rows repeated, so that the sorting and de-duplication of the pair sets is exercised; cutoff 300.

Saved: h, label_list [1, M, 6], test_label_list [1, M', 6], cutoff, the table's columns (row, col, score fp32, score_ranking,
train_edge, test_edge, new_edge) in the table's order, and the counts the script prints (total, total_wo_train,
total_target_edges, total_train_edges, total_test_edges, top_ratio [10], test_edges_in_toplist [10], enrichment [10]).

    python tests/golden/make_golden_predscore.py
"""
import contextlib
import io
import os
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SCRIPT = os.path.join(REF, "sample_kg", "network_prediction", "script")
N, D, SEED, CUTOFF = 40, 8, 49, 300


def case():
    rng = np.random.default_rng(SEED)
    # 780 scores on a grid of 1 / 4096 collide in a plain draw (16 ties at this seed): the rows are drawn one at a time and a
    # row whose scores against the rows before it would tie with a score already there (or with each other) is drawn again
    h, seen = np.zeros((0, D), np.float32), set()
    while len(h) < N:
        r = (rng.integers(-64, 65, D) / 64.0).astype(np.float32)
        new = (h @ r).tolist()
        if len(set(new)) == len(new) and not seen.intersection(new):
            h, seen = np.concatenate([h, r[None]]), seen.union(new)
    m32 = h @ h.T
    assert np.array_equal(m32.astype(np.float64), h.astype(np.float64) @ h.astype(np.float64).T), "H H^T is not exact in fp32"
    iu = np.triu_indices(N, 1)
    assert len(np.unique(m32[iu])) == N * (N - 1) // 2, "tied pair scores"
    pick = rng.permutation(len(iu[0]))[:150]
    pairs = np.stack([iu[0][pick], iu[1][pick]], 1)

    def rows(p, repeats):
        p = np.concatenate([p, p[:repeats]])
        flip = rng.random(len(p)) < 1.0 / 3.0
        a, b = np.where(flip, p[:, 1], p[:, 0]), np.where(flip, p[:, 0], p[:, 1])
        neg = rng.integers(0, N, len(p))
        return np.stack([a, np.full(len(p), 2), b, a, np.zeros(len(p), np.int64), neg], 1)[rng.permutation(len(p))]

    return h, m32, np.asarray([rows(pairs[:120], 12)], np.int32), np.asarray([rows(pairs[120:], 5)], np.int32)


def main():
    import joblib
    sys.path.insert(0, SCRIPT)
    import predscore as P
    h, m32, label_list, test_label_list = case()
    names = {i: "n%d" % i for i in range(N)}
    text = io.StringIO()
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(text):
        dataset, result = os.path.join(tmp, "dataset.jbl"), os.path.join(tmp, "result.jbl")
        joblib.dump({"label_list": label_list, "test_label_list": test_label_list}, dataset)
        joblib.dump({"prediction_data": m32[None]}, result)
        test_pairs = P.build_test_label_pairs(dataset, "infer", 0)
        target_pairs = P.build_target_label_pairs(dataset, "infer")
        top = P.sort_prediction_score(result, "infer", target_pairs, test_pairs, CUTOFF, True, names)
        total_list = []
        P.convert(top, set(target_pairs), set(test_pairs), names, True, total_list)        # one process: the list as it is
        col = lambda k: [l[k] for l in total_list]
        table = P.process_table(col(1), col(2), col(3), col(4), col(0), col(5), col(6), col(7))
        P.enrichment(target_pairs, test_pairs, table, True, names)
    out = text.getvalue()
    one = lambda pat: int(re.search(pat + r": (\d+)", out).group(1))
    many = lambda pat, conv: np.asarray([conv(x) for x in re.findall(pat + r": ([0-9.e+-]+)", out)])
    np.savez_compressed(
        os.path.join(HERE, "g10_predscore.npz"), h=h, label_list=label_list, test_label_list=test_label_list,
        cutoff=np.int64(CUTOFF), row=table["row"].to_numpy(np.int32), col=table["col"].to_numpy(np.int32),
        score=table["score"].to_numpy(np.float32), score_ranking=table["score_ranking"].to_numpy(np.int64),
        train_edge=table["train_edge"].to_numpy(np.int64), test_edge=table["test_edge"].to_numpy(np.int64),
        new_edge=table["new_edge"].to_numpy(np.int64), total=one(r"#total as scored"), total_wo_train=one(r"#total_w/o_train_edges"),
        total_target_edges=one(r"#total_target_edges"), total_train_edges=one(r"#total_train_edges"),
        total_test_edges=one(r"#total_test_edges"), top_ratio=many(r"#top_ratio", int),
        test_edges_in_toplist=many(r"#test_edges_in_toplist", int), enrichment=many(r"#test edges enrichment top[0-9.]+%", float))


if __name__ == "__main__":
    main()
