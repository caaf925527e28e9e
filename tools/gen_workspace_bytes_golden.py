#!/usr/bin/env python3
"""Record what every *_workspace_bytes query of include/kgcn_hip.h answers over a table of shapes ->
tests/golden/workspace_bytes.json, which tests/test_workspace_queries.py holds the library to.

The queries are host functions: no GPU is needed.  The sizes are behaviour of the ABI (callers allocate exactly what a query
says), so the file is recorded from the library as it was BEFORE a change to the host code that sizes or carves a workspace:

    make -C <checkout of the earlier commit>/kgcn_amd/csrc
    KGCN_HIP_LIB=<that checkout>/kgcn_amd/csrc/libkgcn_hip.so python tools/gen_workspace_bytes_golden.py

and is not regenerated to make a failing test pass.  Per query the table holds the shapes of the example model configurations,
the smallest legal shape, a zero and a negative size, and one shape per refusal (-1) of the queries that refuse.

A call is [name, args]; an argument is an integer, or for kgcn_gcn_stack_bwd_workspace_bytes a list of layers
[kind, din, dout] (kind 0 GraphConv, 1 Dense, 2 batch normalisation) that stands for the (layers, num_layers) pair.

DEVICE_DEPENDENT names the queries that are left out: their answer includes the temporary storage rocPRIM asks for its sorts and
scans, which depends on the device the process sees (and is another number again on a machine without one), so no file recorded on
one machine holds on the next.  None of them is a packed layout; tests/test_gpu_workspace_contract.py holds their entry points to
their own query's answer on the GPU.
"""
import json
import os
import sys

DEVICE_DEPENDENT = frozenset("kgcn_%s_workspace_bytes" % n for n in (
    "coo_pack", "csr_pad4", "linkpred", "pair_rank", "wl_rank", "graph_runs", "graph_gram", "rank_pairs", "wl_rank_copies",
    "graph_runs_copies", "binary_metrics"))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")

# rows of a dense layer in the configs: 128 graphs x 50 nodes (model_multitask.py), sparse.py's 4,457 rows, the 16,384 rows at
# which the one-pass backward starts, the 100 x 132 nodes of model_gin.py
ROWS = (6400, 4457, 16384, 13200)
# (din, dout) of the configs' dense layers: wide, narrow-in, read-out, 50-wide, the fused GraphConv's 64 x 64
WIDTHS = ((256, 256), (81, 256), (132, 256), (256, 50), (50, 50), (64, 64), (256, 12), (64, 2), (75, 64))
STACKS = (
    [[0, 7, 24], [0, 24, 13], [1, 13, 64]],                                     # tests/stack_cases.py: relu_chain
    [[0, 5, 64], [2, 64, 64], [1, 64, 64], [0, 64, 33], [2, 33, 33], [0, 33, 20], [1, 20, 8], [2, 8, 8]],   # eight_layers
    [[0, 75, 64], [2, 64, 64], [0, 64, 64], [2, 64, 64], [1, 64, 32]],          # the GCN of example_model/model.py
    [[1, 1, 1]],                                                                # the smallest list
)
# conv-pool of the sequence encoder: (batch, length, symbols, embed, kernel, filters, pool); limits of include/kgcn_hip.h
SEQ_OK = ((100, 1000, 25, 16, 4, 10, 4), (128, 8192, 1024, 32, 8, 64, 8), (1, 1, 1, 1, 1, 1, 1), (0, 8, 5, 4, 3, 2, 2),
          (-3, 8, 5, 4, 3, 2, 2), (2, 4, 2, 1, 1, 1, 2), (600, 64, 25, 8, 3, 16, 2),
          (262144, 8192, 5, 4, 3, 2, 2))                       # (the query does not look at batch x length)
SEQ_REFUSED = ((2, 0, 5, 4, 3, 2, 2), (2, 8193, 5, 4, 3, 2, 2), (2, 8, 5, 0, 3, 2, 2), (2, 8, 5, 33, 3, 2, 2), (2, 8, 5, 4, 3, 0, 2),
               (2, 8, 5, 4, 3, 65, 2), (2, 8, 5, 4, 0, 2, 2), (2, 8, 5, 4, 9, 2, 2), (2, 8, 5, 4, 3, 2, 0), (2, 8, 5, 4, 3, 2, 9),
               (2, 8, 0, 4, 3, 2, 2), (2, 8, 1025, 4, 3, 2, 2))
# the protein-sequence CNN: (batch, length, in_dim, kernel, filters, pool)
CONV1D_OK = ((32, 1000, 32, 8, 64, 2), (32, 500, 64, 8, 128, 2), (32, 250, 128, 8, 256, 2), (1, 1, 1, 1, 1, 1), (0, 8, 3, 3, 2, 2),
             (2, 4, 1, 1, 1, 2), (2, 3, 5, 2, 3, 4), (2048, 8192, 1024, 8, 1024, 8), (100, 8192, 21, 3, 1024, 1))
CONV1D_REFUSED = ((-1, 8, 3, 3, 2, 2), (2, 0, 3, 3, 2, 2), (2, 8193, 3, 3, 2, 2), (2, 8, 0, 3, 2, 2), (2, 8, 1025, 3, 2, 2),
                  (2, 8, 3, 3, 0, 2), (2, 8, 3, 3, 1025, 2), (2, 8, 3, 0, 2, 2), (2, 8, 3, 9, 2, 2), (2, 8, 3, 3, 2, 0),
                  (2, 8, 3, 3, 2, 9), (2 ** 31 - 1, 8192, 1024, 3, 2, 2), (2 ** 31 - 1, 1, 1, 1, 1, 1))


def calls():
    c = []

    def add(name, *shapes):
        c.extend([name, list(s) if isinstance(s, (tuple, list)) else [s]] for s in shapes)

    add("kgcn_dense_wgrad_workspace_bytes", *[(m, i, o) for m in ROWS for i, o in WIDTHS],
        (1, 1, 1), (5, 3, 2), (31, 7, 16), (1 << 22, 256, 256), (0, 3, 2), (-1, 3, 2), (5, 0, 2), (5, 3, -2))
    add("kgcn_dense_dx_dact_dot_workspace_bytes", *[(m, i) for m in ROWS for i in (132, 256)], (1, 1), (0, 132), (-5, 132), (16384, 0))
    add("kgcn_dense_fwd_workspace_bytes", *WIDTHS, *[(o, i) for i, o in WIDTHS], (1, 1), (192, 129), (191, 129), (0, 256), (256, -1))
    add("kgcn_graphconv_bwd_workspace_bytes", (128, 64, 64), (100, 75, 64), (2049, 64, 64), (65, 12, 36), (67, 5, 6), (1, 1, 1),
        (0, 64, 64), (-1, 64, 64), (2, 0, 64), (2, 64, -3))
    add("kgcn_gcn_stack_bwd_workspace_bytes", *[(t, s) for s in STACKS for t in (100, 1, 1024, 1025, 5000)],
        (0, STACKS[0]), (-2, STACKS[0]), (40, []))
    add("kgcn_graph_bn_workspace_bytes", 64, 50, 256, 33, 5, 1, 0, -4)
    add("kgcn_graph_maxpool_bwd_workspace_bytes", (100, 50, 64), (128, 132, 32), (2, 3, 3), (1, 1, 1), (0, 3, 3), (2, -1, 3), (2, 3, 0))
    add("kgcn_gat_workspace_bytes", (100, 50, 64), (128, 132, 32), (2, 3, 3), (1, 1, 1), (0, 3, 3), (2, 0, 3), (2, 3, -1))
    add("kgcn_gin_aggregate_bwd_workspace_bytes", (100, 132, 81), (100, 132, 256), (2, 3, 3), (1, 1, 1), (300, 1, 1), (0, 3, 3),
        (-2, 3, 3), (2, 3, 0))
    add("kgcn_gram_workspace_bytes", 64, 32, 5, 1, 0, -1)
    add("kgcn_dot_workspace_bytes", 1 << 20, 3379200, 1, 0, -1)
    add("kgcn_loss_workspace_bytes", 128, 100, 4457, 1, 256, 257, 1 << 20, 0, -7)
    add("kgcn_csr_gather_workspace_bytes", 128, 100, 1, 256, 257, 100000, 0, -1)
    add("kgcn_batch_assemble_workspace_bytes", 128, 100, 1, 256, 257, 100000, 0, -1)
    add("kgcn_ragged_workspace_bytes", 128, 100, 1, 256, 257, 100000, 0, -1)
    add("kgcn_ragged_gather_bwd_workspace_bytes", 64, 50, 256, 1, 0, -2)
    add("kgcn_vae_recon_workspace_bytes", (128, 1, 64), (100, 4, 32), (2, 2, 1), (1, 1, 1), (1024, 8, 64), (1025, 8, 64), (5000, 2, 16),
        (0, 2, 4), (2, 0, 4), (2, 2, 0), (-1, 2, 4))
    add("kgcn_seq_convpool_workspace_bytes", *SEQ_OK, *SEQ_REFUSED)
    add("kgcn_seq_lstm_workspace_bytes", (100, 250, 10, 32), (128, 1000, 64, 64), (2, 2, 3, 2), (1, 1, 1, 1), (0, 0, 3, 2), (-1, -1, 3, 2),
        (2, 2, 0, 2), (2, 2, 3, 0), (2, 2, -3, 2), (2, 2, 3, -2))
    add("kgcn_conv1d_pool_workspace_bytes", *CONV1D_OK, *CONV1D_REFUSED)
    add("kgcn_cpi_ig_workspace_bytes", (2, 512, 3, 101), (16, 64, 12, 51), (2, 3, 2, 2), (1, 1, 1, 1), (0, 512, 3, 101), (2, 0, 3, 101),
        (2, 512, -1, 101), (2, 512, 3, 0))
    # the sort-and-rank workspaces that hold no rocPRIM scratch (256-byte arrays from a rounded base): sizes and rounding as they are
    add("kgcn_attr_scale_workspace_bytes", (150000, 64), (3, 2), (1, 1), (100000, 4096), (0, 2), (-1, 2), (3, 0), (3, -1), (3, 4097),
        (2 ** 31 - 1, 2))
    add("kgcn_svm_workspace_bytes", (1, 4), (300, 188), (1, 1), (0, 4), (1, 0), (-1, 4))
    add("kgcn_lp_workspace_bytes", (5, 1, 2), (5000, 12, 24), (1, 1, 1), (0, 1, 2), (5, 0, 2), (5, 1, 0), (-1, 1, 2))
    return c


def answer(lib_module, name, args):
    """the query's answer for one call of the table (layer lists become the kgcn_stack_layer array and its length)"""
    out = []
    for a in args:
        if isinstance(a, list):
            layers = (lib_module.StackLayer * max(len(a), 1))()
            for l, (kind, din, dout) in zip(layers, a):
                l.kind, l.din, l.dout = kind, din, dout
            out += [layers, len(a)]
        else:
            out.append(a)
    return int(getattr(lib_module.lib, name)(*out))


def main():
    import warnings
    warnings.simplefilter("ignore", RuntimeWarning)            # the override's own warning: swapping the library is the point
    from kgcn_amd import _lib
    table = calls()
    queries = sorted(n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes"))
    queries = [n for n in queries if n not in DEVICE_DEPENDENT]
    missing = sorted(set(queries) - {n for n, _ in table})
    if missing:
        sys.exit("no shapes for %s" % ", ".join(missing))
    rows = [[name, args, answer(_lib, name, args)] for name, args in table]
    with open(GOLDEN, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("%d answers of %d queries from %s -> %s" % (len(rows), len(queries), _lib.LIB_PATH, GOLDEN))


if __name__ == "__main__":
    main()
