"""The dense layer's host-side routing answers over a grid that straddles every boundary of the route chains (CPU only: the
reporting functions are host code and the library loads without a GPU).

tests/golden/dense_routes.json was recorded from the library as it was BEFORE the routes of csrc/dense.hip were gathered into
fwd_route / wgrad_route; it is never regenerated from the code under test.  Every entry must match exactly: which kernel a call
takes decides summation order, workspace sizes are what callers allocate."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_routes.json")

# column of the recording -> arguments the function takes, out of (m, din, dout)
QUERIES = {
    "mfma_products_0": lambda lib, m, i, o: lib.kgcn_dense_mfma_products(0, m, i, o),
    "mfma_products_1": lambda lib, m, i, o: lib.kgcn_dense_mfma_products(1, m, i, o),
    "mfma_products_2": lambda lib, m, i, o: lib.kgcn_dense_mfma_products(2, m, i, o),
    "fwd_workspace_bytes": lambda lib, m, i, o: lib.kgcn_dense_fwd_workspace_bytes(i, o),
    "wgrad_workspace_bytes": lambda lib, m, i, o: lib.kgcn_dense_wgrad_workspace_bytes(m, i, o),
    "wgrad_dact_supported": lambda lib, m, i, o: lib.kgcn_dense_wgrad_dact_supported(i, o),
    "bwd_supported": lambda lib, m, i, o: lib.kgcn_dense_bwd_supported(m, i, o),
    "dx_dact_gather_supported": lambda lib, m, i, o: lib.kgcn_dense_dx_dact_gather_supported(m, i, o),
    "dx_dact_dot_supported": lambda lib, m, i, o: lib.kgcn_dense_dx_dact_dot_supported(m, i, o),
    "dx_dact_dot_workspace_bytes": lambda lib, m, i, o: lib.kgcn_dense_dx_dact_dot_workspace_bytes(m, i),
}


def test_dense_routing_answers_equal_the_recording():
    from kgcn_amd import _lib      # not at import time: collection must not load the library before torch has loaded its HIP runtime
    with open(GOLDEN) as f:
        rec = json.load(f)
    assert rec["m"] == [1023, 1024, 4095, 4096, 16383, 16384]
    assert rec["din"] == [2, 16, 31, 32, 50, 64, 65, 81, 96, 97, 128, 129, 256, 320, 324]
    assert rec["dout"] == [2, 16, 17, 50, 64, 65, 128, 129, 252, 256, 300]
    assert sorted(rec["columns"]) == sorted(QUERIES)
    shapes = [(m, i, o) for m in rec["m"] for i in rec["din"] for o in rec["dout"]]
    assert len(rec["rows"]) == len(shapes) == 990
    wrong = []
    for (m, i, o), row in zip(shapes, rec["rows"]):
        for name, want in zip(rec["columns"], row):
            got = QUERIES[name](_lib.lib, m, i, o)
            if got != want:
                wrong.append((name, m, i, o, want, got))
    assert not wrong, "%d of %d answers changed, first: %r" % (len(wrong), 990 * len(QUERIES), wrong[:8])
