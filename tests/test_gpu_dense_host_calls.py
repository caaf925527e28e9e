"""The host protocol of the dense layer (kgcn_amd/ops.py: _Dense, _DenseStacked, _DenseGather, _GinDense, the one-pass backward and the
read-out Functions) against a recording of the code as it was BEFORE its four copies were folded into one helper per step.

tools/dense_call_trace.py ran a grid of public calls -- every shape, activation, requires_grad pattern, weight state and module
switch that chooses another branch -- on an MI355X against that earlier ops.py, twice, with `ops.lib` replaced by a forwarding
proxy: tests/golden/dense_host_calls.json holds, per case, every library call in order (queries included, pointer arguments
reduced to null / non-null) and the SHA-256 of every output and gradient.  The dense family has no floating-point atomics and the
two recordings agreed in full, so no hash is left out.  The test replays the grid and asks for the same calls with the same
operands in the same order, and the same bits.  The file is never regenerated from the code under test."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dense_call_trace as trace  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(ROOT, "tests", "golden", "dense_host_calls.json")) as _fh:
    GOLDEN = json.load(_fh)["cases"]
_data = []                       # the seeded operands, generated once for all groups


def test_golden_file_holds_the_whole_grid():
    assert [(g, n) for g, n, _, _ in trace.grid()] == [(c["group"], c["name"]) for c in GOLDEN]
    assert all(c["calls"] and c["hashes"] for c in GOLDEN)
    trace.check_expectations()


@pytest.mark.parametrize("group", trace.GROUPS)
def test_same_library_calls_and_bits_as_recorded(group):
    import torch
    from kgcn_amd import ops
    if not _data:
        _data.append(trace.Data(torch.device("cuda:0")))
    saved = {k: getattr(ops, k) for k in ("wgrad_dact_fusion", "dense_bwd_fusion", "enabled_weight_tables", "side_stream_wgrad")}
    try:
        got = trace.run_cases(ops, groups=(group,), data=_data[0])    # (every case sets its switches and puts them back)
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
    want = [c for c in GOLDEN if c["group"] == group]
    assert [c["name"] for c in got] == [c["name"] for c in want]
    for c, w in zip(got, want):          # (a hash the two recordings disagreed on is not in the file: none at present)
        c["hashes"] = {k: v for k, v in c["hashes"].items() if k in w["hashes"]}
    report = []
    bad_calls, bad_hashes = trace.diff(want, got, out=report.append)
    assert not bad_calls and not bad_hashes, "\n".join(report[:40])
