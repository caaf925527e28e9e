#!/usr/bin/env python3
"""sample_kg/network_prediction/run_enrichment.sh <gcn|distmult|ip> on the MI355X path: script/predscore.py --train --mode
infer on the result of examples/train_linkpred.py.  Reads the node rows H (`output` of <result dir>/test_edge_result.npz; for
distmult also `relation_w`) and the label lists of the fixture (tests/golden/g8_kg_linkpred.npz), ranks all node pairs on the
device (kgcn_amd.predscore.rank_links: the [N, N] prediction is neither read nor formed), prints the summary and the ten
enrichment lines, and writes score_<method>.txt, test_<method>.graph.tsv and train_<method>.graph.tsv into the result dir.

    python examples/enrich_linkpred.py <gcn|distmult|ip> [result dir (result_<method>)] [--cutoff 1500000] [--node names.csv]
                                       [--relation r (distmult: the relation ranked; default the fixture's `interaction`)]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import predscore  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("method", choices=("gcn", "distmult", "ip"))
ap.add_argument("result_dir", nargs="?", default=None)
ap.add_argument("--cutoff", type=int, default=1500000)                 # run_enrichment.sh
ap.add_argument("--node", default=None, help="one node name per line (dataset_node.csv); default: the node ids")
ap.add_argument("--relation", type=int, default=None)
a = ap.parse_args()
out_dir = a.result_dir or "result_%s" % a.method
dev = torch.device("cuda:0")
z = np.load(os.path.join(ROOT, "tests", "golden", "g8_kg_linkpred.npz"))
res = np.load(os.path.join(out_dir, "test_edge_result.npz"))
h = torch.as_tensor(res["output"], dtype=torch.float32, device=dev)
w = None
if a.method == "distmult":
    if "relation_w" not in res.files:
        sys.exit("%s/test_edge_result.npz has no relation_w: rerun examples/train_linkpred.py distmult" % out_dir)
    r = int(z["relation_ids"][2]) if a.relation is None else a.relation
    w = torch.as_tensor(res["relation_w"][r], dtype=torch.float32, device=dev)
    print("ranking relation %d" % r)
elif a.relation is not None:
    sys.exit("--relation is for distmult")
result = predscore.rank_links(h, z["label_list"], z["test_label_list"], w=w, cutoff=a.cutoff)
print("\n".join(result.lines()))
paths = [os.path.join(out_dir, n % a.method) for n in ("score_%s.txt", "test_%s.graph.tsv", "train_%s.graph.tsv")]
predscore.write_score_table(result, paths[0], a.node)
predscore.write_label_sets(result, paths[1], paths[2], a.node)
print("%d entries -> %s; label sets -> %s, %s" % (result.score.numel(), paths[0], paths[1], paths[2]))
