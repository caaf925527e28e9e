#!/usr/bin/env python3
"""One public SpMM entry-point call per row of a grid that straddles every boundary of the route chain in csrc/spmm.hip: the
recorder behind tests/golden/spmm_routes.json and the parent-against-HEAD comparison of profiles/r10_spmm_routes.txt.

  run (GPU box, as the program of a kernel trace):
      rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/spmm_route_driver.py run DIR/rows.json
    every row: seeded operands, ONE call, SHA-256 of the output, then a marker launch (act_kernel) that separates the rows
    in the trace.  rows.json holds, per row, the host-side facts of the call (what kgcn_spmm_route_query takes) and the hash.
  merge (anywhere):  python tools/spmm_route_driver.py merge DIR/rows.json TRACE.csv OUT.json
    attaches kernel name, template arguments, grid (workgroups), workgroup size and LDS bytes from the trace to every row.
  compare (anywhere):  python tools/spmm_route_driver.py compare A.json B.json
  golden (anywhere):  python tools/spmm_route_driver.py golden MERGED.json tests/golden/spmm_routes.json

The golden file is recorded from the library as it was BEFORE the routes were gathered into spmm_route (KGCN_HIP_LIB points
the binding at that build); it is never regenerated from the code under test."""
import csv
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F_DACT, F_SELF, F_DOT, F_FANOUT = 1, 2, 4, 8
SQUARE = (10, 16, 17, 32, 33, 50, 64, 65)
WIDTHS = (7, 30, 32, 50, 64, 128, 256, 512, 1024, 1028)
T = 3


def grid():
    """(name, variant, container spec, nch, d, operand offset in floats)"""
    rows = []
    for n in SQUARE:
        for d in WIDTHS:
            for v in ("plain", "dact", "gin", "gin_bwd"):
                rows.append((v, ("batch", n, n, 3 * n), 1, d, 0))
            for c in (2, 8):
                for v in ("act", "fanout", "fanout_dact"):
                    rows.append((v, ("batch", n, n, 2 * n), c, d, 0))
    for n in (10, 17, 32, 50, 65):                                # 8- and 4-byte aligned operands: views offset by 2 and 1 floats
        for d in WIDTHS:
            for v in ("plain", "dact"):
                for off in (2, 1):
                    rows.append((v, ("batch", n, n, 3 * n), 1, d, off))
    for n in (10, 32, 64):
        for d in (30, 32, 50, 64, 256):
            for v in ("act", "fanout_dact"):
                for off in (2, 1):
                    rows.append((v, ("batch", n, n, 2 * n), 2, d, off))
    for k in (120, 150):                                          # rectangular: the 64 KiB fallback out of the slices route
        for v in ("plain", "dact"):
            rows.append((v, ("batch", 20, k, 60), 1, 128, 0))
    for nnz in (1270, 1280):                                      # the 20 KiB tile limit (10 x 256 floats + entries)
        rows.append(("plain", ("batch", 10, 10, nnz), 1, 256, 0))
    for nnz in (350, 365):                                        # the 53 KiB limit of the four-wave tile
        rows.append(("plain", ("batch", 50, 50, nnz), 1, 256, 0))
    for nnz in (4950, 4960):                                      # the 40 KiB limit of the channel loop
        rows.append(("act", ("batch", 10, 10, nnz), 2, 32, 0))
        rows.append(("fanout", ("batch", 10, 10, nnz), 2, 32, 0))
    for r in (84, 720, 33000):                                    # one-graph containers, with and without a block table
        for blocks in (1, 0):
            for d in (32, 50, 256, 1028):
                for v in ("plain", "dact", "gin"):
                    rows.append((v, ("one", r, blocks), 1, d, 0))
    return rows


def facts(variant, spec, nch, d):
    """The host-side facts of a row's call: descriptor scalars, strides, flags."""
    if spec[0] == "batch":
        _, m, k, nnz = spec
        if variant in ("gin_bwd", "fanout", "fanout_dact"):
            m, k = k, m                                           # these read the transposed containers
        desc = dict(num_graphs=T, rows=m, cols=k, max_nnz=[nnz] * nch, num_blocks=0, block_rows_max=0)
    else:
        _, r, blocks = spec
        desc = dict(num_graphs=1, rows=r, cols=r, max_nnz=[3 * r], num_blocks=(r + 63) // 64 if blocks else 0,
                    block_rows_max=75 if blocks else 0)
    m, k = desc["rows"], desc["cols"]
    f = dict(desc, nch=nch, d=d, flags=0)
    if variant in ("fanout", "fanout_dact"):
        f.update(rhs_ld=d, rhs_gs=k * d, cs=d, out_ld=nch * d, out_gs=m * nch * d,
                 flags=F_FANOUT | (F_DACT if variant == "fanout_dact" else 0))
    elif variant == "act":
        f.update(rhs_ld=nch * d, rhs_gs=k * nch * d, cs=d, out_ld=d, out_gs=m * d)
    else:
        f.update(rhs_ld=d, rhs_gs=k * d, cs=0, out_ld=d, out_gs=m * d,
                 flags={"plain": 0, "dact": F_DACT, "gin": F_SELF, "gin_bwd": F_SELF | F_DOT}[variant])
    return f


# ---- run: the calls ------------------------------------------------------------------------------------------------------
def run(out_path):
    import numpy as np
    import torch
    from kgcn_amd._lib import lib, check, current_stream, LIB_PATH
    from kgcn_amd.batched_csr import BatchedCSR, BatchedAdjacency
    dev = torch.device("cuda:0")
    cache = {}

    def container(spec, nch):
        key = (spec, nch)
        if key in cache:
            return cache[key]
        rng = np.random.default_rng(sum(spec[1:]) * 131 + nch)
        chans = []
        for c in range(nch):
            if spec[0] == "batch":
                _, m, k, nnz = spec
                g = np.repeat(np.arange(T), nnz)
                r = rng.integers(0, m, size=T * nnz)
                cc = rng.integers(0, k, size=T * nnz)
                a = BatchedCSR.from_arrays(g, r, cc, rng.standard_normal(T * nnz).astype(np.float32), T, m, k, device=dev)
            else:
                _, n, blocks = spec
                r = np.repeat(np.arange(n), 3)
                cc = np.clip(r + rng.integers(-5, 6, size=r.size), 0, n - 1)
                a = BatchedCSR.from_arrays(np.zeros(r.size, np.int64), r, cc, rng.standard_normal(r.size).astype(np.float32), 1,
                                           n, n, device=dev)
                if blocks:
                    bp = np.minimum(np.arange((n + 63) // 64 + 1) * 64, n).astype(np.int32)
                    a.block_ptr = torch.from_numpy(bp).to(dev)
                    a.block_rows_max = 75
            chans.append(a)
        cache[key] = BatchedAdjacency(chans)
        return cache[key]

    def view(rng, shape, off):
        n = int(np.prod(shape))
        buf = torch.from_numpy(rng.standard_normal(n + 4).astype(np.float32)).to(dev)
        return buf, buf[off:off + n]

    marker = torch.zeros(64, device=dev)
    recs = []
    for i, (variant, spec, nch, d, off) in enumerate(grid()):
        f = facts(variant, spec, nch, d)
        adj = container(spec, nch)
        m, k, tt = f["rows"], f["cols"], f["num_graphs"]
        rng = np.random.default_rng(1000 + i)
        s = current_stream()
        keep = []
        if variant in ("fanout", "fanout_dact"):
            hold, g = view(rng, (tt * k, d), off)
            hold2, ao = view(rng, (tt * k, d), off)
            hold3, out = view(rng, (tt * m, nch * d), off)
            act = 1 if variant == "fanout_dact" else 0
            check(lib.kgcn_bconv_fanout_f32(adj.desc_array(True), nch, g.data_ptr(), ao.data_ptr() if act else None, d, k * d, d, act,
                                            out.data_ptr(), nch * d, m * nch * d, d, s), variant)
            keep = [out]
        elif variant == "act":
            hold, rhs = view(rng, (tt * k, nch * d), off)
            hold3, out = view(rng, (tt * m, d), off)
            check(lib.kgcn_bconv_act_f32(adj.desc_array(), nch, rhs.data_ptr(), nch * d, k * nch * d, d, d, out.data_ptr(), d, m * d,
                                         1, s), variant)
            keep = [out]
        elif variant in ("plain", "dact"):
            hold, rhs = view(rng, (tt * k, d), off)
            hold2, ao = view(rng, (tt * k, d), off)
            hold3, out = view(rng, (tt * m, d), off)
            a = adj.channels[0].desc()
            if variant == "plain":
                check(lib.kgcn_bspmm_f32(a, rhs.data_ptr(), d, k * d, d, out.data_ptr(), d, m * d, 0.0, s), variant)
            else:
                check(lib.kgcn_bspmm_dact_f32(a, rhs.data_ptr(), ao.data_ptr(), d, k * d, d, 3, out.data_ptr(), d, m * d, 0.0, s),
                      variant)
            keep = [out]
        else:
            hold, x = view(rng, (tt * m, d), 0)
            hold2, g = view(rng, (tt * m, d), 0)
            hold3, out = view(rng, (tt * m, d), 0)
            eps = torch.full((1,), 0.37, device=dev)
            if variant == "gin":
                check(lib.kgcn_gin_aggregate_f32(adj.desc_array(), 1, x.data_ptr(), d, eps.data_ptr(), out.data_ptr(), s), variant)
                keep = [out]
            else:
                wsb = lib.kgcn_gin_aggregate_bwd_workspace_bytes(tt, m, d)
                ws = torch.zeros(max(wsb // 4, 1), device=dev)
                deps = torch.zeros(1, device=dev)
                check(lib.kgcn_gin_aggregate_bwd_f32(adj.desc_array(True), 1, g.data_ptr(), d, eps.data_ptr(), x.data_ptr(),
                                                     out.data_ptr(), deps.data_ptr(), ws.data_ptr(), wsb, s), variant)
                keep = [out, deps]
        check(lib.kgcn_act_fwd_f32(marker.data_ptr(), 64, 0, marker.data_ptr(), s), "marker")
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in keep:
            h.update(t.cpu().numpy().tobytes())
        recs.append(dict(f, variant=variant, align={0: 16, 2: 8, 1: 4}[off], sha256=h.hexdigest()))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump({"library": os.path.relpath(LIB_PATH, ROOT), "rows": recs}, fh)
    print("%d rows -> %s (library %s)" % (len(recs), out_path, LIB_PATH))


# ---- merge: kernel, template arguments, grid, workgroup, LDS out of the trace ------------------------------------------------
NAME = re.compile(r"kgcn::((?:spmm|bconv)_\w+?)_kernel(?:<([^>]*)>)?")


def merge(rows_path, trace_path, out_path):
    with open(rows_path) as fh:
        doc = json.load(fh)
    with open(trace_path, newline="") as fh:
        trace = [{k.lower(): v for k, v in r.items()} for r in csv.DictReader(fh)]
    trace.sort(key=lambda r: int(r["start_timestamp"]))
    per_row, cur = [], []
    for r in trace:
        name = r["kernel_name"]
        if "act_kernel" in name:
            per_row.append(cur)
            cur = []
            continue
        mt = NAME.search(name)
        if mt and mt.group(1) != "spmm_values_grad":
            wg = int(r["workgroup_size_x"])
            targs = [{"true": 1, "false": 0}.get(a.strip(), a.strip()) for a in (mt.group(2) or "").split(",") if a.strip()]
            cur.append(dict(kernel=mt.group(1), targs=[int(a) for a in targs], grid=int(r["grid_size_x"]) // wg, workgroup=wg,
                            lds=int(r["lds_block_size"])))      # (the trace counts the grid in work-items)
    assert len(per_row) == len(doc["rows"]), "%d marker launches for %d rows" % (len(per_row), len(doc["rows"]))
    for row, ks in zip(doc["rows"], per_row):
        row["launches"] = ks
    with open(out_path, "w") as fh:
        json.dump(doc, fh)
    print("%d rows, %d launches -> %s" % (len(per_row), sum(map(len, per_row)), out_path))


def compare(a_path, b_path):
    with open(a_path) as fh:
        a = json.load(fh)
    with open(b_path) as fh:
        b = json.load(fh)
    assert len(a["rows"]) == len(b["rows"])
    bad_route = bad_hash = 0
    for i, (ra, rb) in enumerate(zip(a["rows"], b["rows"])):
        if ra["launches"] != rb["launches"]:
            bad_route += 1
            print("row %d launches differ: %r / %r" % (i, ra["launches"], rb["launches"]))
        if ra["sha256"] != rb["sha256"]:
            bad_hash += 1
            print("row %d (%s) output hash differs" % (i, ra["variant"]))
    kinds = {}
    for r in a["rows"]:
        for k in r["launches"]:
            key = "%s<%s>" % (k["kernel"], ",".join(map(str, k["targs"])))
            kinds[key] = kinds.get(key, 0) + 1
    print("%s against %s: %d rows, %d launches, %d instantiations; launches differ in %d rows, output hashes in %d rows"
          % (a["library"], b["library"], len(a["rows"]), sum(len(r["launches"]) for r in a["rows"]), len(kinds), bad_route, bad_hash))
    for k in sorted(kinds):
        print("  %5d  %s" % (kinds[k], k))
    return 1 if bad_route or bad_hash else 0


def golden(merged_path, out_path):
    """The test's file: the call facts and what the trace showed (a fan-out that fell back to one launch per channel keeps all
    of them); no hashes, no LDS bytes (the trace reports them rounded to the allocation granule)."""
    with open(merged_path) as fh:
        doc = json.load(fh)
    cols = ["variant", "num_graphs", "rows", "cols", "max_nnz", "num_blocks", "block_rows_max", "nch", "d", "rhs_ld", "rhs_gs", "cs",
            "out_ld", "out_gs", "align", "flags"]
    rows = []
    for r in doc["rows"]:
        rows.append([r[c] for c in cols] + [[[k["kernel"], k["targs"], k["grid"], k["workgroup"]] for k in r["launches"]]])
    with open(out_path, "w") as fh:
        fh.write('{"columns": %s,\n "rows": [\n' % json.dumps(cols + ["launches"]))
        fh.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        fh.write("\n]}\n")
    print("%d rows -> %s" % (len(rows), out_path))


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else ""
    if cmd == "run":
        run(sys.argv[2])
    elif cmd == "merge":
        merge(*sys.argv[2:5])
    elif cmd == "compare":
        sys.exit(compare(*sys.argv[2:4]))
    elif cmd == "golden":
        golden(*sys.argv[2:4])
    else:
        sys.exit(__doc__)
