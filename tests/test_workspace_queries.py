"""Every *_workspace_bytes query answers what tests/golden/workspace_bytes.json recorded (tools/gen_workspace_bytes_golden.py, run
against the library as it was before the workspace layouts moved into layout functions): callers allocate exactly what a query
says, so a size is behaviour of the ABI.  The queries are host functions; no GPU is needed.  The queries whose answer includes
rocPRIM's temporary storage depend on the device and are not in the file (DEVICE_DEPENDENT of the tool)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_workspace_bytes_golden as G  # noqa: E402


def _golden():
    with open(G.GOLDEN) as f:
        return json.load(f)


def test_the_table_is_the_recorded_one_and_names_every_query():
    from kgcn_amd import _lib
    rows = _golden()
    assert [[n, a] for n, a, _ in rows] == G.calls()
    assert {n for n, _, _ in rows} == {n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")} - G.DEVICE_DEPENDENT
    per_query = {}
    for n, _, v in rows:
        per_query.setdefault(n, []).append(v)
    for n, values in per_query.items():
        assert max(values) > 0 and len(values) >= 5, (n, values)
    for n in ("kgcn_seq_convpool_workspace_bytes", "kgcn_conv1d_pool_workspace_bytes"):
        assert per_query[n].count(-1) == len({"seq": G.SEQ_REFUSED, "conv1d": G.CONV1D_REFUSED}[n.split("_")[1]]), n


def test_every_query_answers_what_it_answered():
    from kgcn_amd import _lib
    wrong = [(n, a, v, got) for n, a, v in _golden() for got in [G.answer(_lib, n, a)] if got != v]
    assert not wrong, wrong[:10]


def test_cpi_ig_pin():
    from kgcn_amd import _lib
    assert _lib.lib.kgcn_cpi_ig_workspace_bytes(2, 512, 3, 101) == 2 * 101 * (512 + 3) * 4
