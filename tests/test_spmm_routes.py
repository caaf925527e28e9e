"""The batched SpMM's host-side route (csrc/spmm.hip, spmm_route, reported by kgcn_spmm_route_query) over a grid that straddles
every boundary of the route chain (CPU only: the query is host code, follows no device pointer, and the library loads without a
GPU).

tests/golden/spmm_routes.json was recorded from the library as it was BEFORE the routes were gathered into spmm_route:
tools/spmm_route_driver.py issued one public entry-point call per row on an MI355X under `rocprofv3 --kernel-trace`, and kernel
name, template arguments, grid and workgroup size were taken from the trace.  It is never regenerated from the code under test.
Every row must match exactly: which kernel a call takes decides summation order."""
import ctypes
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spmm_routes.json")


def query(lib_mod, num_graphs, rows, cols, max_nnz, num_blocks, block_rows_max, nch, d, rhs_ld, rhs_gs, cs, out_ld, out_gs, align,
          flags):
    """kgcn_spmm_route_query on host descriptors whose device pointers are placeholders -> (kernel name, template arguments,
    grid, workgroup, ds, slices, lds bytes)"""
    descs = (lib_mod.CsrBatch * nch)()
    for c in range(nch):
        descs[c] = lib_mod.CsrBatch(num_graphs, rows, cols, max_nnz[c], 0, 0, max_nnz[c] * num_graphs, 0, 0, 0, 0,
                                    8 if num_blocks else 0, num_blocks, block_rows_max)
    r = lib_mod.SpmmRoute()
    lib_mod.check(lib_mod.lib.kgcn_spmm_route_query(descs, nch, d, rhs_ld, rhs_gs, cs, out_ld, out_gs, align, flags, ctypes.byref(r)),
                  "kgcn_spmm_route_query")
    return lib_mod.SPMM_KERNELS[r.kernel], list(r.template_args), r.grid, r.workgroup, r.ds, r.slices, r.lds_bytes


NARGS = {"spmm_tile": 4, "spmm_slices": 1, "spmm_block": 3, "spmm_rows": 4, "spmm_gather": 1, "bconv_loop": 3, "bconv_fanout": 2}


def expected(launch):
    """a launch of the recording as the query names it: the DOT form of the tile kernel is a kernel code of its own"""
    kernel, targs, grid, wg = launch
    assert len(targs) == NARGS[kernel]
    if kernel == "spmm_tile" and targs[3]:
        kernel = "spmm_tile_dot"
    return kernel, targs + [0] * (4 - len(targs)), grid, wg


def test_spmm_routes_equal_the_recording():
    from kgcn_amd import _lib      # not at import time: collection must not load the library before torch has loaded its HIP runtime
    with open(GOLDEN) as f:
        rec = json.load(f)
    cols = rec["columns"]
    assert cols[-1] == "launches" and len(rec["rows"]) == 1144
    seen, wrong = set(), []
    for row in rec["rows"]:
        call = dict(zip(cols, row))
        launches = call.pop("launches")
        variant = call.pop("variant")
        got = query(_lib, **call)
        if call["flags"] & _lib.SPMM_FANOUT and launches[0][0] != "bconv_fanout":
            # the fan-out fell back to one single-channel launch per channel: the query says so, and each of those launches
            # is what the query answers for one channel of the same call without the fan-out flag
            assert len(launches) == call["nch"] and len(set(map(json.dumps, launches))) == 1
            one = dict(call, nch=1, max_nnz=call["max_nnz"][:1], cs=0, flags=call["flags"] & ~_lib.SPMM_FANOUT)
            got = (got[0],) + query(_lib, **one)[:4]
            want = ("none",) + expected(launches[0])
        else:
            assert len(launches) == 1, (variant, call, launches)
            want = expected(launches[0])
            got = got[:4]
        seen.add((want[-4], tuple(want[-3])))
        if got != want:
            wrong.append((variant, call, want, got))
    assert not wrong, "%d of %d rows changed, first: %r" % (len(wrong), len(rec["rows"]), wrong[:4])
    # the grid reaches every kernel of the file and both call variants of the tile kernel
    assert {k for k, _ in seen} == set(_lib.SPMM_KERNELS[1:])


def test_query_argument_checks_and_empty_batches():
    from kgcn_amd import _lib
    d = (_lib.CsrBatch * 1)(_lib.CsrBatch(3, 10, 10, 30, 0, 0, 90, 0, 0, 0, 0, 0, 0, 0))
    r = _lib.SpmmRoute()
    q = _lib.lib.kgcn_spmm_route_query
    assert q(d, 1, 32, 32, 320, 0, 32, 320, 16, 0, ctypes.byref(r)) == 0 and _lib.SPMM_KERNELS[r.kernel] == "spmm_tile"
    assert (list(r.template_args), r.grid, r.workgroup, r.ds, r.slices) == ([8, 4, 1, 0], 3, 64, 32, 1)
    assert r.lds_bytes == 10 * 32 * 4 + 30 * 8 + 11 * 4 + 4                    # tile | entries | row offsets, rounded to 16
    assert q(d, 1, 0, 0, 0, 0, 0, 0, 16, 0, ctypes.byref(r)) == 0 and r.kernel == 0      # d = 0: nothing to launch
    assert q(d, 0, 32, 32, 320, 0, 32, 320, 16, 0, ctypes.byref(r)) != 0
    assert q(d, 9, 32, 32, 320, 0, 32, 320, 16, 0, ctypes.byref(r)) != 0                 # more than one launch takes
    assert q(d, 1, 32, 32, 320, 0, 32, 320, 3, 0, ctypes.byref(r)) != 0                  # alignment: 16, 8 or 4
    assert q(d, 1, -1, 32, 320, 0, 32, 320, 16, 0, ctypes.byref(r)) != 0
    assert q(None, 1, 32, 32, 320, 0, 32, 320, 16, 0, ctypes.byref(r)) != 0
    assert q(d, 1, 32, 32, 320, 0, 32, 320, 16, 0, None) != 0
