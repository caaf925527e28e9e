#!/usr/bin/env python3
"""`kgcn visualize --visualize_type edge_score|edge_loss|node [--visualize_target i] [--graph_distance d]` of
sample_kg/network_prediction on the MI355X path (gcn.py:651-672 -> cal_feature_IG_for_kg, kgcn/visualization.py:389-439): integrated
gradients of one label row's score, of its cost, or of a node's best prediction with respect to the embedded layer, 30 steps,
dumped as <name>-edge.csv / <name>-node.csv per target (the subgraph within graph_distance hops, ig normalised over all nodes).

The data setup is examples/train_linkpred.py's (the BA network of tests/golden/g8_kg_linkpred.npz); the model is trained briefly
here (--epochs, default 1) unless --load names a state dict.  With --visualize_target unset EVERY row of the test label list (every
node for 'node') is attributed, as the reference does: the scaled forwards run once, the targets go through ops.kg_ig in chunks.

    python examples/visualize_linkpred.py [gcn|distmult|ip] --visualize_type edge_score --visualize_target 7
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kgcn_amd import data_util as D, models, train, visualization as V  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("variant", nargs="?", default="gcn", choices=models.LinkPredictionNet.VARIANTS)
ap.add_argument("--visualize_type", default="edge_score", choices=V.KG_VISUALIZE_TYPES)
ap.add_argument("--visualize_target", type=int, default=None)
ap.add_argument("--graph_distance", type=int, default=1)                          # gcn.py:716
ap.add_argument("--visualize_path", default="visualization")
ap.add_argument("--epochs", type=int, default=1)
ap.add_argument("--load", default=None, help="state dict of a trained LinkPredictionNet")
ap.add_argument("--max_dump", type=int, default=None, help="write the csv files of the first n targets only")
args = ap.parse_args()

LR = {"gcn": 0.001, "distmult": 0.01, "ip": 0.001}[args.variant]
dev = torch.device("cuda:0")
z = np.load(os.path.join(ROOT, "tests", "golden", "g8_kg_linkpred.npz"))
data = D.LinkPredictionData({"adj": [(z["adj_idx"], z["adj_val"], np.array([int(z["node_num"])] * 2))], "node": z["node"],
                             "node_num": z["node_num"], "label_list": z["label_list"], "test_label_list": z["test_label_list"]})
graph = data.adjacency(dev)
adj = graph if args.variant == "gcn" else None
feed = D.LinkPredFeed(data.label_list, batch=1000, adjacency=adj, device=dev)

torch.manual_seed(0)
model = models.LinkPredictionNet(args.variant, data.num_nodes, data.num_relations, seed=1234, device=dev)
model(None, adj, feed=feed)
if args.load:
    model.load_state_dict(torch.load(args.load, map_location=dev))
else:
    opt = train.TFAdam(model.parameters(), lr=LR)
    model.bind_step(opt._t_dev)
    step = train.GraphedTrainStep(model, opt, model.loss, feed, None, None, feed=feed)
    rng = np.random.RandomState(1234)
    for epoch in range(args.epochs):
        feed.shuffle(rng)
        cost = sum(float(step.replay()[0]) for _ in range(feed.steps_per_epoch))
        print("epoch %3d  training cost %.5f" % (epoch, cost), flush=True)

t0 = time.time()
results = V.linkpred_integrated_gradients(model, adj, data.test_label_list, args.visualize_type, target=args.visualize_target,
                                          divide_number=30)
torch.cuda.synchronize()
print("%d targets attributed in %.2f s" % (len(results), time.time() - t0))
for r in results[:5]:
    print("target %d  vis_nodes %s  sum_of_IG %.6f  check (end - start) %.6f" % (r["target"], r["vis_nodes"], r["sum_of_ig"],
                                                                                 r["end_score"] - r["start_score"]))
files = V.dump_kg(results if args.max_dump is None else results[:args.max_dump], graph, args.visualize_path, args.graph_distance,
                  visualize_type=args.visualize_type)
print("%d file pairs -> %s (first: %s, %s)" % ((len(files), args.visualize_path) + tuple(os.path.basename(f) for f in files[0])))
