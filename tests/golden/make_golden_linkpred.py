#!/usr/bin/env python3
"""Generate tests/golden/g8_kg_linkpred.npz by IMPORTING the reference's preprocessing script in place
(sample_kg/network_prediction/script/preprocessing_link_pred.py; nothing of it is copied, only the arrays its functions return).

A seeded 80/20 split of data/ba_model.graph.tsv (np.random.default_rng(0) permutation of the lines) is written to two temporary
.graph.tsv files, then the script's __main__ block is followed with its own load_graph, build_label_list and build_adjs under
np.random.seed(0).  The block iterates Python sets of strings (an order that changes with the interpreter's hash seed); the
edge and node lists are sorted before they reach the random draws, so the file is reproducible.

Saved (int32): adj_idx [nnz, 2], adj_val [nnz], node_num, label_list [1, M, 6], test_label_list [1, M', 6], node [1, N], and
the relation ids (negative, self, interaction).

    python tests/golden/make_golden_linkpred.py
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SAMPLE = os.path.join(REF, "sample_kg", "network_prediction")
SEED = 0


def split_lines(lines, seed=SEED, rate=0.2):
    """The seeded split: the last int(n rate) lines of a default_rng(seed) permutation are the test edges."""
    order = np.random.default_rng(seed).permutation(len(lines))
    n_test = int(len(lines) * rate)
    return [lines[i] for i in order[:len(lines) - n_test]], [lines[i] for i in order[len(lines) - n_test:]]


def main():
    sys.path.insert(0, os.path.join(SAMPLE, "script"))
    import preprocessing_link_pred as P
    lines = open(os.path.join(SAMPLE, "data", "ba_model.graph.tsv")).read().splitlines()
    train, test = split_lines(lines)
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        paths = []
        for name, part in (("train", train), ("test", test)):
            paths.append(os.path.join(tmp, "dataset.%s.graph.tsv" % name))
            with open(paths[-1], "w") as f:
                f.write("\n".join(part) + "\n")
        np.random.seed(SEED)
        labels = {"negative": 0, "self": 1}
        train_edges, train_nodes, labels = P.load_graph([paths[0]], labels)
        test_edges, test_nodes, labels = P.load_graph([paths[1]], labels)
    all_nodes = sorted(train_nodes | test_nodes)
    mp = {el: i for i, el in enumerate(all_nodes)}
    conv = lambda es: sorted((mp[e[0]], labels[e[1]], mp[e[2]]) for e in es)
    train_edges, test_edges = conv(train_edges), conv(test_edges)
    target_nodes = sorted(mp[e] for e in (train_nodes | test_nodes))
    self_edges = [(i, labels["self"], i) for i in range(len(all_nodes))]
    label_list = P.build_label_list(target_nodes, train_edges, len(train_edges))
    test_label_list = P.build_label_list(target_nodes, test_edges, len(test_edges))
    adjs = P.build_adjs(train_edges, self_edges, len(all_nodes))
    N = len(all_nodes)
    np.savez_compressed(
        os.path.join(HERE, "g8_kg_linkpred.npz"),
        adj_idx=np.asarray(adjs[0][0], np.int32), adj_val=np.asarray(adjs[0][1], np.int32), node_num=np.int32(N),
        node=np.arange(N, dtype=np.int32)[None], label_list=np.asarray([label_list], np.int32),
        test_label_list=np.asarray([test_label_list], np.int32),
        relation_ids=np.asarray([labels["negative"], labels["self"], labels["interaction"]], np.int32))


if __name__ == "__main__":
    main()
