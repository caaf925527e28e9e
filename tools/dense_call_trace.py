#!/usr/bin/env python3
"""What the dense layer's host code in kgcn_amd/ops.py asks of the library: every C call of one public call and its backward pass,
in order, over a grid that reaches every branch of _Dense, _DenseStacked, _DenseGather, _GinDense, _dense_bwd_fused and the
read-out Functions.  The recorder behind tests/golden/dense_host_calls.json and profiles/r11_dense_host_calls.txt.

  record (GPU box):   python tools/dense_call_trace.py record OUT.json [--ops FILE] [--lines]
    every case: seeded operands, `ops.lib` replaced by a forwarding proxy for the duration of the case, the calls with every pointer
    argument (by _lib.SIGNATURES) reduced to "P" / "N" (non-null / null) -- queries (*_supported, *_workspace_bytes,
    kgcn_reduce_defer, kgcn_reduce_pending) included -- and, after a synchronise, the SHA-256 of every output and gradient.
    --ops FILE: the cases run against that file in place of kgcn_amd/ops.py (another commit's, with this tree's library; only the
    public API is used, so the same grid runs against both).  --lines: the line of ops.py that issued each call.
  compare (anywhere): python tools/dense_call_trace.py compare A.json B.json
  golden (anywhere):  python tools/dense_call_trace.py golden A.json B.json tests/golden/dense_host_calls.json
    A and B: two recordings of the same ops.py in one GPU call; a hash that differs between them is left out (and printed), a call
    list never is.
  sites (anywhere):   python tools/dense_call_trace.py sites A.json OPS_FILE
    the `check(lib.` call sites of the dense and read-out Functions of OPS_FILE with the cases of A (recorded with --lines) that
    reach each; exit status 1 if one is not reached.

The golden file is recorded from ops.py as it was BEFORE the four copies of the protocol were folded; it is never regenerated from
the code under test."""
import contextlib
import ctypes
import hashlib
import importlib.util
import json
import os
import re
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = ("dense_narrow", "dense_1100", "dense_16500", "dense_16500x50", "dense_switches", "dense_stacked", "dense_gather_60",
          "dense_gather_500", "dense_gather_1800", "gin_dense", "readouts")
ACTS = (None, "relu", "sigmoid")
# the answers of the library's route queries the grid was laid out for, as (rows, din, dout) -> (forward workspace?, one-pass
# backward, gathered dX, dot dX, d-activation inside the weight gradient); checked before a recording, not assumed
EXPECT = {(300, 50, 50): (0, 0, 0, 0, 0), (1100, 256, 256): (1, 0, 1, 0, 1), (16500, 256, 256): (1, 1, 1, 1, 1),
          (16500, 256, 50): (1, 0, 0, 0, 0), (1100, 260, 256): (1, 0, 1, 0, 1), (600, 50, 50): (0, 0, 0, 0, 0),
          (5000, 256, 256): (1, 0, 1, 0, 1), (18000, 256, 256): (1, 1, 1, 1, 1), (17000, 256, 256): (1, 1, 1, 1, 1),
          (20480, 160, 256): (1, 1, 1, 1, 1), (3000, 256, 256): (1, 0, 1, 0, 1)}


def load_ops(path=None):
    """kgcn_amd.ops, or the file `path` loaded as a module of the package (its relative imports resolve to this tree)."""
    import kgcn_amd
    if path is None:
        return kgcn_amd.ops
    spec = importlib.util.spec_from_file_location("kgcn_amd._ops_traced", os.path.abspath(path))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def check_expectations():
    from kgcn_amd._lib import lib
    for (m, din, dout), want in EXPECT.items():
        got = (int(lib.kgcn_dense_fwd_workspace_bytes(din, dout) > 0), lib.kgcn_dense_bwd_supported(m, din, dout),
               lib.kgcn_dense_dx_dact_gather_supported(m, din, dout), lib.kgcn_dense_dx_dact_dot_supported(m, din, dout),
               lib.kgcn_dense_wgrad_dact_supported(din, dout))
        assert got == want, "the grid no longer straddles the routes at %r: %r, laid out for %r" % ((m, din, dout), got, want)


# ---- the proxy -------------------------------------------------------------------------------------------------------------
class Recorder:
    """Stands in for ops.lib: forwards every call and appends [name, arguments...] to self.calls."""

    def __init__(self, real, ops_file=None):
        from kgcn_amd._lib import SIGNATURES
        self._real, self._sigs, self._file = real, SIGNATURES, ops_file
        self.calls, self.lines = [], []

    @staticmethod
    def _is_pointer(t):
        return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))

    @staticmethod
    def _null(a):
        if a is None:
            return True
        if isinstance(a, int):
            return a == 0
        if isinstance(a, ctypes.c_void_p):
            return not a.value
        return False                                              # a ctypes array or structure: an address

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        sig = self._sigs.get(name)
        if sig is None:
            return fn

        def call(*args):
            rec = [name]
            for a, t in zip(args, sig[1]):
                rec.append(("N" if self._null(a) else "P") if self._is_pointer(t) else (a.value if hasattr(a, "value") else a))
            self.calls.append(rec)
            if self._file is not None:
                f = sys._getframe(1)
                while f is not None and f.f_code.co_filename != self._file:
                    f = f.f_back
                self.lines.append(f.f_lineno if f is not None else 0)
            return fn(*args)
        return call


# ---- operands --------------------------------------------------------------------------------------------------------------
class Data:
    """Seeded operands by (tag, shape), generated once and cloned into every case."""

    def __init__(self, device):
        self.device, self.cache = device, {}

    def t(self, tag, *shape, scale=1.0):
        import numpy as np
        import torch
        key = (tag, shape)
        if key not in self.cache:
            rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
            self.cache[key] = torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32)).to(self.device)
        return self.cache[key]

    def leaf(self, tag, *shape, grad=True, scale=1.0):
        return self.t(tag, *shape, scale=scale).clone().requires_grad_(grad)

    def adjacency(self, T, N):
        """one channel: a ring with self loops in every graph"""
        import numpy as np
        from kgcn_amd.batched_csr import BatchedAdjacency, BatchedCSR
        key = ("adj", T, N)
        if key not in self.cache:
            g = np.repeat(np.arange(T), 3 * N)
            r = np.tile(np.repeat(np.arange(N), 3), T)
            c = (r + np.tile(np.array([-1, 0, 1]), T * N)) % N
            self.cache[key] = BatchedAdjacency([BatchedCSR.from_arrays(g, r, c, np.ones(g.size, np.float32), T, N, N, device=self.device)])
        return self.cache[key]


@contextlib.contextmanager
def switches(ops, **values):
    prev = {k: getattr(ops, k) for k in values}
    try:
        for k, v in values.items():
            setattr(ops, k, v)
        yield
    finally:
        for k, v in prev.items():
            setattr(ops, k, v)


def weights(ops, D, din, dout, bias, warm, grad_w=True, grad_b=True, bias_shape=None):
    """(w, bias): plain tensors ("cold": no table exists for them), or parameters that one forward registered ("warm": the
    refresh in front of the recorded call splits their tables)."""
    import torch
    w = D.t("w", din, dout, scale=din ** -0.5).clone()
    b = D.t("b", *(bias_shape or (dout,)), scale=0.1).clone() if bias else None
    if not warm:
        return w.requires_grad_(grad_w), None if b is None else b.requires_grad_(grad_b)
    w = torch.nn.Parameter(w, requires_grad=grad_w)
    b = None if b is None else torch.nn.Parameter(b, requires_grad=grad_b)
    with torch.no_grad():
        ops.dense(D.t("x", 4, din), w, None)
    return w, b


# ---- the grid: (group, name, switches, function(ops, D) -> (call, wanted)) -------------------------------------------------------
# `call()` makes the public call and its backward pass and returns the tensors to hash by name; everything in front of it
# (operands, the registering forward of a warm weight) is not recorded.
def _backward(outs, grads):
    import torch
    pairs = [(o, g) for o, g in zip(outs, grads) if g is not None]
    if pairs and any(o.requires_grad for o, _ in pairs):
        torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])


def _grads(named):
    return {k + ".grad": v.grad for k, v in named.items() if v is not None and v.grad is not None}


def dense_case(m, din, dout, act, rg, warm, defer=False, stacked_weight=False):
    def make(ops, D):
        x = D.leaf("x", m, din, grad=bool(rg[0]))
        if stacked_weight:                                        # a computed (non-leaf) weight: [w; bias; 0] of stack_rows
            w0, b0 = weights(ops, D, din - 4, dout, True, False, bias_shape=(1, dout))
            params = {"w": w0, "b": b0}
        else:
            w, b = weights(ops, D, din, dout, rg[2] is not None, warm, bool(rg[1]), bool(rg[2]))
            params = {"w": w, "b": b}
        g = D.t("g", m, dout)

        def call():
            if stacked_weight:
                y = ops.dense(x, ops.stack_rows(w0, b0, w0.new_zeros((3, dout))), None, activation=act)
            else:
                y = ops.dense(x, w, b, activation=act)
            with ops.deferred_reductions(root=y) if defer else contextlib.nullcontext():
                _backward([y], [g])
            return dict({"y": y}, **_grads(dict(params, x=x)))
        return call
    return make


def stacked_case(m, din, dout, act, warm):
    def make(ops, D):
        import torch
        rows = din + 4
        x = D.t("x", m, rows)
        w, b = D.t("w", din, dout, scale=din ** -0.5).clone(), D.t("b", 1, dout, scale=0.1).clone()
        if warm:
            w, b = torch.nn.Parameter(w), torch.nn.Parameter(b)
            with torch.no_grad():
                ops.dense_stacked(x, w, b)
        else:
            w.requires_grad_(True), b.requires_grad_(True)
        g = D.t("g", m, dout)

        def call():
            y = ops.dense_stacked(x, w, b, activation=act)
            assert y.grad_fn.name().startswith("_DenseStacked") == warm, y.grad_fn.name()
            _backward([y], [g])
            return dict({"y": y}, **_grads({"w": w, "b": b}))
        return call
    return make


def gather_case(T, N, din, dout, act, incoming, joined, x_grad, warm=False, bias=True):
    def make(ops, D):
        import torch
        x = D.leaf("x", T, N, din, grad=x_grad)
        w, b = weights(ops, D, din, dout, bias, warm)
        gy = D.t("g", T, N, dout) if "y" in incoming else None
        gp = D.t("gp", T, dout) if "p" in incoming else None
        gcat = D.t("gcat", T, 2 * dout)

        def call():
            if joined:                                            # two read-outs side by side; the second block's gradient is strided
                buf = torch.zeros((T, 2 * dout), device=x.device)
                other = ops.graph_gather_into(D.t("other", T, N, dout), buf, 0)
                y, p = ops.dense_gather(x, w, b, activation=act, join=buf, join_col=dout)
                cat = ops.join_columns(buf, [other, p])
                _backward([y, cat], [gy, gcat])
                return dict({"y": y, "cat": cat}, **_grads({"x": x, "w": w, "b": b}))
            y, p = ops.dense_gather(x, w, b, activation=act)
            _backward([y, p], [gy, gp])
            return dict({"y": y, "pooled": p}, **_grads({"x": x, "w": w, "b": b}))
        return call
    return make


def gin_case(T, N, din, dout, act, w_grad, warm, expect_fused):
    def make(ops, D):
        x = D.t("x", T, N, din)
        eps = D.leaf("eps", 1, scale=0.3)
        adj = D.adjacency(T, N)
        w, b = weights(ops, D, din, dout, True, warm, w_grad, w_grad)
        g = D.t("g", T, N, dout)

        def call():
            y = ops.gin_dense(x, eps, adj, w, b, activation=act)
            assert y.grad_fn.name().startswith("_GinDense") == expect_fused, y.grad_fn.name()
            _backward([y], [g])
            return dict({"y": y}, **_grads({"eps": eps, "w": w, "b": b}))
        return call
    return make


def readout_case(kind, B, N, d, incoming):
    def make(ops, D):
        import torch
        x = D.leaf("x", B, N, d)
        gx = D.t("g", B, N, d) if "x" in incoming else None
        gp = D.t("gp", B, d) if "p" in incoming else None

        def call():
            if kind == "gather":
                p = ops.graph_gather(x)
                _backward([p], [gp])
                return dict({"pooled": p}, **_grads({"x": x}))
            if kind == "tee":
                y, p = ops.graph_gather_tee(x)
                _backward([y, p], [gx, gp])
                return dict({"y": y, "pooled": p}, **_grads({"x": x}))
            buf = torch.zeros((B, d + 4), device=x.device)
            p = ops.graph_gather_into(x, buf, 4)
            _backward([p], [gp])
            return dict({"buf": buf}, **_grads({"x": x}))
        return call
    return make


RG = ((1, 1, 1), (0, 1, 1), (1, 0, 0), (1, 1, None))              # requires_grad of (x, w, bias); None: no bias


def grid():
    rows = []

    def add(group, name, make, **sw):
        rows.append((group, name, sw, make))

    for group, (m, din, dout) in (("dense_narrow", (300, 50, 50)), ("dense_1100", (1100, 256, 256)),
                                  ("dense_16500", (16500, 256, 256)), ("dense_16500x50", (16500, 256, 50))):
        for act in ACTS:
            for rg in RG:
                for warm in (False, True):
                    add(group, "dense %dx%dx%d %s rg=%s %s" % (m, din, dout, act, "".join("-" if r is None else str(r) for r in rg),
                                                               "warm" if warm else "cold"), dense_case(m, din, dout, act, rg, warm))
    S = "dense_switches"
    for m in (1100, 16500):
        add(S, "dense %d relu no one-pass backward" % m, dense_case(m, 256, 256, "relu", RG[0], True), dense_bwd_fusion=False)
        add(S, "dense %d relu x fixed, no d-activation in the weight gradient" % m, dense_case(m, 256, 256, "relu", RG[1], True),
            wgrad_dact_fusion=False)
        add(S, "dense %d relu no weight tables" % m, dense_case(m, 256, 256, "relu", RG[0], True), enabled_weight_tables=False)
        add(S, "dense %d sigmoid x fixed no weight tables" % m, dense_case(m, 256, 256, "sigmoid", RG[1], True),
            enabled_weight_tables=False)
    add(S, "dense 16500 relu side stream", dense_case(16500, 256, 256, "relu", RG[0], True), side_stream_wgrad=True)
    add(S, "dense 16500x256x50 relu x fixed side stream", dense_case(16500, 256, 50, "relu", RG[1], False), side_stream_wgrad=True)
    for rg in (RG[0], RG[1]):
        add(S, "dense 1100 relu stack_rows weight rg=%d" % rg[0], dense_case(1100, 260, 256, "relu", rg, False, stacked_weight=True))
    for act in (None, "relu"):
        add(S, "dense 16500 %s warm deferred" % act, dense_case(16500, 256, 256, act, RG[0], True, defer=True))
    add(S, "dense 1100 relu x fixed warm deferred", dense_case(1100, 256, 256, "relu", RG[1], True, defer=True))
    for warm in (True, False):
        for act in (None, "relu"):
            for fusion in (True, False):
                add("dense_stacked", "dense_stacked 1100 %s %s dact-fusion=%d" % (act, "warm" if warm else "cold", fusion),
                    stacked_case(1100, 256, 256, act, warm), wgrad_dact_fusion=fusion)
    for group, (T, N, din, dout) in (("dense_gather_60", (60, 10, 50, 50)), ("dense_gather_500", (500, 10, 256, 256)),
                                     ("dense_gather_1800", (1800, 10, 256, 256))):
        for act in ("relu", "sigmoid", None):
            for incoming in ("y", "p", "yp"):
                for joined in ((False,) if incoming == "y" else (False, True)):
                    for x_grad in (True, False):
                        add(group, "dense_gather %dx%dx%dx%d %s d%s%s x=%d" % (T, N, din, dout, act, incoming, " joined" if joined else "",
                                                                              x_grad), gather_case(T, N, din, dout, act, incoming, joined, x_grad))
        for act in ("relu", None):                                 # warm weights: the table forms of the forward and of the plain dX
            for incoming in ("y", "yp"):
                add(group, "dense_gather %dx%dx%dx%d %s d%s warm" % (T, N, din, dout, act, incoming),
                    gather_case(T, N, din, dout, act, incoming, False, True, warm=True))
        add(group, "dense_gather %dx%dx%dx%d relu dyp no bias" % (T, N, din, dout), gather_case(T, N, din, dout, "relu", "yp", False, True, bias=False))
    for incoming in ("p", "yp"):                                   # 4 nodes: below the one-pass backward's n_nodes >= 8
        add("dense_gather_1800", "dense_gather 4500x4x256x256 relu d%s" % incoming, gather_case(4500, 4, 256, 256, "relu", incoming, False, True))
    for T, N, din, dout in ((1700, 10, 256, 256), (640, 32, 160, 256)):
        for w_grad in (True, False):
            for fusion in (True, False):
                for warm in (False, True):
                    add("gin_dense", "gin_dense %dx%dx%dx%d relu w=%d one-pass=%d %s" % (T, N, din, dout, w_grad, fusion, "warm" if warm else "cold"),
                        gin_case(T, N, din, dout, "relu", w_grad, warm, True), dense_bwd_fusion=fusion)
    add("gin_dense", "gin_dense 1700x10x256x256 sigmoid", gin_case(1700, 10, 256, 256, "sigmoid", True, False, True))
    add("gin_dense", "gin_dense 300x10x256x256 relu (two ops)", gin_case(300, 10, 256, 256, "relu", True, False, False))
    for kind in ("gather", "tee", "into"):
        for B, N, d in ((8, 5, 12), (60, 10, 50)):
            for incoming in (("x", "p", "xp") if kind == "tee" else ("p",)):
                add("readouts", "graph_gather_%s %dx%dx%d d%s" % (kind, B, N, d, incoming), readout_case(kind, B, N, d, incoming))
    return rows


# ---- record ----------------------------------------------------------------------------------------------------------------
def run_cases(ops, groups=None, lines=False, data=None):
    """-> [{"group", "name", "calls", "hashes"[, "lines"]}] of the grid's cases (of `groups`) against the module `ops`."""
    import torch
    D = data or Data(torch.device("cuda:0"))
    ops_file = ops.__file__ if lines else None
    recs = []
    for group, name, sw, make in grid():
        if groups is not None and group not in groups:
            continue
        with switches(ops, **sw):
            call = make(ops, D)
            ops.weight_tables.refresh()                           # a step begins: tables of the registered weights, use counts cleared
            real, rec = ops.lib, Recorder(ops.lib, ops_file)
            ops.lib = rec
            try:
                kept = call()
                torch.cuda.synchronize()
            finally:
                ops.lib = real
        hashes = {k: hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest() for k, t in sorted(kept.items())}
        r = {"group": group, "name": name, "calls": rec.calls, "hashes": hashes}
        if lines:
            r["lines"] = rec.lines
        recs.append(r)
        del kept, call
    return recs


def record(out_path, ops_path=None, lines=False):
    from kgcn_amd._lib import LIB_PATH
    check_expectations()
    ops = load_ops(ops_path)
    recs = run_cases(ops, lines=lines)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump({"ops": os.path.relpath(ops.__file__, ROOT), "library": os.path.relpath(LIB_PATH, ROOT), "cases": recs}, fh)
    print("%d cases, %d calls -> %s (ops %s)" % (len(recs), sum(len(r["calls"]) for r in recs), out_path, ops.__file__))


def _load(path):
    with open(path) as fh:
        return json.load(fh)


def diff(a_cases, b_cases, out=print):
    """-> (cases whose call lists differ, hashes that differ); a hash only one side has counts as different."""
    assert [c["name"] for c in a_cases] == [c["name"] for c in b_cases], "the two recordings do not hold the same cases"
    bad_calls, bad_hashes = [], []
    for ca, cb in zip(a_cases, b_cases):
        if ca["calls"] != cb["calls"]:
            bad_calls.append(ca["name"])
            out("%s: calls differ" % ca["name"])
            for i in range(max(len(ca["calls"]), len(cb["calls"]))):
                x = ca["calls"][i] if i < len(ca["calls"]) else None
                y = cb["calls"][i] if i < len(cb["calls"]) else None
                if x != y:
                    out("   call %d: %r\n        against %r" % (i, x, y))
        for k in sorted(set(ca["hashes"]) | set(cb["hashes"])):
            if ca["hashes"].get(k) != cb["hashes"].get(k):
                bad_hashes.append((ca["name"], k))
                out("%s: hash of %s differs" % (ca["name"], k))
    return bad_calls, bad_hashes


def compare(a_path, b_path):
    a, b = _load(a_path), _load(b_path)
    bad_calls, bad_hashes = diff(a["cases"], b["cases"])
    print("%s against %s: %d cases, %d calls, %d hashes; call lists differ in %d cases, %d hashes differ"
          % (a["ops"], b["ops"], len(a["cases"]), sum(len(c["calls"]) for c in a["cases"]),
             sum(len(c["hashes"]) for c in a["cases"]), len(bad_calls), len(bad_hashes)))
    return 1 if bad_calls or bad_hashes else 0


def golden(a_path, b_path, out_path):
    a, b = _load(a_path), _load(b_path)
    bad_calls, bad_hashes = diff(a["cases"], b["cases"])
    assert not bad_calls, "the two recordings of one ops.py disagree on their calls: %r" % bad_calls
    with open(out_path, "w") as fh:
        fh.write('{"cases": [\n')
        rows = []
        for c in a["cases"]:
            hashes = {k: v for k, v in c["hashes"].items() if (c["name"], k) not in bad_hashes}
            rows.append(json.dumps({"group": c["group"], "name": c["name"], "calls": c["calls"], "hashes": hashes}, separators=(",", ":")))
        fh.write(",\n".join(rows))
        fh.write("\n]}\n")
    print("%d cases -> %s; %d hashes left out %r" % (len(a["cases"]), out_path, len(bad_hashes), bad_hashes))


SITE_SCOPES = ("_dense_bwd_fused", "_Dense", "_DenseStacked", "_DenseGather", "_GinDense", "_Gather", "_GatherTee", "_GatherInto")


def sites(rec_path, ops_path):
    """The call sites (`check(lib.NAME(` inside SITE_SCOPES) of ops_path and the cases of the recording that reach each."""
    doc = _load(rec_path)
    src = open(ops_path).read().split("\n")
    found, scope = [], None
    for i, line in enumerate(src, 1):
        mt = re.match(r"(?:class|def) (\w+)", line)
        if mt:
            scope = mt.group(1)
        elif line and not line[0].isspace() and not line.startswith(("#", ")")):
            scope = None
        mt = re.search(r"check\(lib\.(\w+)\(", line)
        if mt and scope in SITE_SCOPES:
            found.append((i, scope, mt.group(1)))
    reached = {s: [] for s in found}
    for c in doc["cases"]:
        for call, ln in zip(c["calls"], c["lines"]):
            # (the frame's line is that of the call expression, at most two lines below the `check(` it sits in)
            for s in found:
                if s[2] == call[0] and 0 <= ln - s[0] <= 2 and c["name"] not in reached[s]:
                    reached[s].append(c["name"])
    missing = 0
    for s in found:
        names = reached[s]
        missing += not names
        print("%s:%d  %s  %s  -- %d cases%s" % (os.path.basename(ops_path), s[0], s[1], s[2], len(names),
                                                 "" if names else "  NOT REACHED"))
        for n in names[:4]:
            print("        %s" % n)
        if len(names) > 4:
            print("        ... and %d more" % (len(names) - 4))
    print("%d call sites, %d not reached" % (len(found), missing))
    return 1 if missing else 0


if __name__ == "__main__":
    argv = sys.argv[1:]
    cmd = argv[0] if argv else ""
    if cmd == "record":
        opts = argv[2:]
        record(argv[1], opts[opts.index("--ops") + 1] if "--ops" in opts else None, "--lines" in opts)
    elif cmd == "compare":
        sys.exit(compare(*argv[1:3]))
    elif cmd == "golden":
        golden(*argv[1:4])
    elif cmd == "sites":
        sys.exit(sites(*argv[1:3]))
    else:
        sys.exit(__doc__)
